"""GPU side of the clip search (A7c): tg_group_params_clip against the numpy
restatement of its contract (tests/clip_ref.py), the Quantizer path through
gptq_fwrd and packing, the end-to-end gain on the pinned problem, and the
harness switch.

Bars.  choice equals the restatement's except on ambiguous groups (two
distinct candidates within 1e-9 relative at the minimum; at most 1 % of a
case's groups, and test_clip_host.py shows there are none on these inputs);
scale / zero are bit-equal to the restatement's candidate `choice`; the
objectives are within 1e-12 relative of the restatement's float64 sums (a
sum of at most 28,672 non-negative terms in another order differs by a few
1e-14), and exactly 0 where those are 0.
"""
import json
import os

import numpy as np
import pytest
import torch

import clip_ref
from abi_helpers import DEV, SENTINEL, dev, logical, outside_intact, padded
from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu
GRID, STEPS = clip_ref.GRID, clip_ref.STEPS


@pytest.fixture(scope="module")
def lib():
    from gptq_svd_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def g():
    import gptq_svd_amd.gptq_utils as g
    return g


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def run_clip(lib, pW, m, n, stride, h, group, bits, sym, grid=GRID, steps=STEPS):
    """-> scale, zero (m, G) f32, choice (m, G) i32, objective (m, G, 2) f64;
    one sentinel element after each output must survive."""
    G = n // (n if group <= 0 else group)
    sz = torch.full((2, m * G + 1), SENTINEL, dtype=torch.float32, device=DEV)
    ch = torch.full((m * G + 1,), -77, dtype=torch.int32, device=DEV)
    ob = torch.full((2 * m * G + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    dh = None if h is None else dev(np.array(h))     # the shared inputs are read-only
    lib.call("tg_group_params_clip", lib.stream(), pW, m, n, stride, lib.ptr(dh), group, bits,
             int(sym), grid, steps, lib.ptr(sz[0]), lib.ptr(sz[1]), lib.ptr(ch), lib.ptr(ob))
    sz, ch, ob = sz.cpu().numpy(), ch.cpu().numpy(), ob.cpu().numpy()
    assert sz[0, -1] == SENTINEL and sz[1, -1] == SENTINEL and ch[-1] == -77 and ob[-1] == SENTINEL
    return (sz[0, :-1].reshape(m, G).copy(), sz[1, :-1].reshape(m, G).copy(),
            ch[:-1].reshape(m, G).copy(), ob[:-1].reshape(m, G, 2).copy())


def close(got, ref):
    return np.all(np.where(ref == 0, got == 0, np.abs(got - ref) <= 1e-12 * ref))


@pytest.mark.parametrize("bits", clip_ref.BITS)
@pytest.mark.parametrize("shape", clip_ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_clip_parity(lib, shape, bits):
    m, n, group = shape
    for sym in (False, True):
        for weighted in (False, True):
            W, h, ref = clip_ref.case(m, n, group, bits, sym, weighted)
            amb = clip_ref.ambiguous(ref)
            assert amb.sum() <= 0.01 * amb.size
            for ld, lead in ((n, 0), (n + 3, 1)):
                tag = f"{shape} bits={bits} sym={sym} weighted={weighted} ld={ld}"
                pW, bW = padded(W, ld, lead)
                s, z, ch, ob = run_clip(lib, pW, m, n, ld, h, group, bits, sym)
                assert bits_equal(logical(bW, W.shape, ld, lead), W), tag
                assert outside_intact(bW, W.shape, ld, lead), tag
                assert ch.min() >= 0 and ch.max() <= STEPS, tag
                bad = (ch != ref["choice"]) & ~amb
                assert not bad.any(), (tag, int(bad.sum()), ch[bad][:4], ref["choice"][bad][:4])
                at = lambda a: np.take_along_axis(a, ch[:, :, None].astype(np.int64),
                                                  axis=2)[:, :, 0]
                assert bits_equal(s, at(ref["s"])), tag
                assert bits_equal(z, at(ref["z"])), tag
                assert close(ob[:, :, 0], ref["J"][:, :, 0]), tag
                assert close(ob[:, :, 1], at(ref["J"])), tag
                assert np.all(ob[:, :, 1] <= ob[:, :, 0]), tag


@pytest.mark.parametrize("shape", clip_ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_steps0_is_group_params(lib, shape):
    """steps = 0 is tg_group_params bit for bit, with and without weights."""
    m, n, group = shape
    W = clip_ref.clip_input(m, n, group)
    G = n // (n if group <= 0 else group)
    dW = dev(W)
    for bits in clip_ref.BITS:
        h = clip_ref.clip_weights(n, bits)
        for sym in (False, True):
            out = torch.empty((2, m, G), dtype=torch.float32, device=DEV)
            lib.call("tg_group_params", lib.stream(), lib.ptr(dW), m, n, n, group, bits, int(sym),
                     lib.ptr(out[0]), lib.ptr(out[1]))
            o = out.cpu().numpy()
            for hh in (None, h):
                s, z, ch, ob = run_clip(lib, lib.ptr(dW), m, n, n, hh, group, bits, sym,
                                        grid=100, steps=0)
                tag = f"{shape} bits={bits} sym={sym} weighted={hh is not None}"
                assert bits_equal(s, o[0]) and bits_equal(z, o[1]), tag
                assert not ch.any() and bits_equal(ob[:, :, 0], ob[:, :, 1]), tag


@pytest.mark.parametrize("shape", [(37, 330, 110), (5, 384, 128), (2, 8256, -1)],
                         ids=lambda s: "x".join(map(str, s)))
def test_two_calls_are_bit_identical(lib, shape):
    m, n, group = shape
    W, h, _ = clip_ref.case(m, n, group, 3, False, True)
    dW = dev(np.array(W))
    a = run_clip(lib, lib.ptr(dW), m, n, n, h, group, 3, False)
    b = run_clip(lib, lib.ptr(dW), m, n, n, h, group, 3, False)
    for x, y in zip(a, b):
        assert bits_equal(x, y)


@pytest.mark.parametrize("shape", [(37, 330, 110), (7, 256, 32)],
                         ids=lambda s: "x".join(map(str, s)))
def test_row_shards_are_bit_identical(lib, shape):
    """Rows are independent: a call on a slice of the rows gives those rows'
    results of the whole call (what row sharding over ranks relies on)."""
    m, n, group = shape
    W, h, _ = clip_ref.case(m, n, group, 4, False, True)
    dW = dev(np.array(W))
    whole = run_clip(lib, lib.ptr(dW), m, n, n, h, group, 4, False)
    for r0, r1 in ((0, m // 3), (m // 3, m)):
        part = run_clip(lib, lib.ptr(dW[r0:r1]), r1 - r0, n, n, h, group, 4, False)
        for x, y in zip(whole, part):
            assert bits_equal(x[r0:r1], y)


@pytest.mark.parametrize("bits,sym", [(3, True), (4, False)])
def test_quantizer_clip_through_gptq_fwrd(g, bits, sym):
    """Scales from the search drive gptq_fwrd and packing like any others."""
    from gptq_svd_amd.qlinear import dequantize_packed
    m, n, group = 64, 256, 128
    rng = np.random.default_rng(bits)
    W = (rng.standard_t(4, (m, n)) * 0.02).astype(np.float32)
    U = np.triu(rng.standard_normal((n, n)) * 0.02)
    U[np.arange(n), np.arange(n)] = 1.0 + np.abs(rng.standard_normal(n))
    perm = rng.permutation(n).astype(np.int64)
    h = rng.lognormal(0.0, 1.0, n)
    q = g.Quantizer(bits, group, sym, clip_search=True, col_weight=torch.from_numpy(h))
    Wq, k = g.gptq_fwrd(dev(W), dev(U.astype(np.float32)), q, dev(perm), block_size=128)
    assert k == n
    ref = clip_ref.clip_search(W, h.astype(np.float32), bits, group, sym)
    ch = q.clip_choice.cpu().numpy()
    assert ch.shape == (m, n // group) and (ch != 0).any()       # the search does move groups
    assert np.array_equal(ch, ref["choice"]) or clip_ref.ambiguous(ref)[ch != ref["choice"]].all()
    ob = q.clip_objective.cpu().numpy()
    assert ob.shape == (m, n // group, 2) and np.all(ob[:, :, 1] <= ob[:, :, 0])
    Wq = Wq.cpu().numpy()
    scale = q.scale.squeeze(-1).cpu().numpy()
    zero = q.zero.squeeze(-1).cpu().numpy()
    off = 2 ** (bits - 1) if sym else 0
    codes = q.codes.cpu().numpy().astype(np.int64) - off
    lo, hi = clip_ref.qrange(bits, sym)
    assert codes.min() >= lo and codes.max() <= hi
    gi = np.arange(n) // group
    grid_w = (codes.astype(np.float32) - zero[:, gi]) * scale[:, gi]
    assert bits_equal(grid_w.astype(np.float32), Wq)
    qw, qz, sc = g.pack_quantized(q)
    assert sc.dtype == torch.float32
    back = dequantize_packed(qw, qz, sc, bits, group, torch.float32).cpu().numpy()
    assert bits_equal(back, Wq)


def test_weighted_search_helps_end_to_end(g):
    """test_clip_host.py's experiment on the GPU path: 3-bit sym g128, energy
    rule 1e-4, block 128.  The CPU oracle gives 0.70; the margin allows for
    near-tie code differences between the GPU solve and LAPACK's."""
    bits, group, sym = 3, 128, True
    X, W = clip_ref.quality_problem(seed=11)
    acc = g.HessianAccumulator(X.shape[1], DEV)
    acc.add_batch(dev(X))
    H = acc.get_hessian()
    R, _, perm = g.process_hessian_alt(H, 1e-4, "energy")
    dW = dev(W)

    def solve(**kw):
        q = g.Quantizer(bits, group, sym, **kw)
        Wq, _ = g.gptq_fwrd(dW, R, q, perm, block_size=128)
        return clip_ref.proxy_error(W, Wq.cpu().numpy(), X)

    plain = solve()
    clipped = solve(clip_search=True, col_weight=torch.diagonal(H))
    print(f"proxy error: min/max {plain:.5f}, weighted search {clipped:.5f}, "
          f"ratio {clipped / plain:.3f}")
    assert clipped < 0.85 * plain


def tiny(d):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    cfg = Qwen3Config(**json.loads(str(d["config"])))
    cfg._attn_implementation = "eager"
    m = Qwen3ForCausalLM(cfg).float().eval()
    m.load_state_dict({k[len("init/"):]: torch.from_numpy(d[k]) for k in d
                       if k.startswith("init/")})
    return m.to(DEV)


def test_harness_clip_search(tmp_path):
    """quantize_model(clip_search=True, pack=True) on the tiny random Qwen3:
    weights on their grids, the clip numbers in layer_stats, the settings in
    results.json and quantize_config.json; clip_search=False changes nothing."""
    from gptq_svd_amd.export import read_quantized
    from gptq_svd_amd.harness import quantize_model, run_and_record
    from gptq_svd_amd.qlinear import dequantize_packed
    d = load_golden(golden_names("h_")[0])
    bits, group = int(d["bits"]), int(d["group"])
    ids = [torch.from_numpy(r[None]) for r in d["ids"]]
    kw = dict(mode=str(d["mode"]), w_bits=bits, group_size=group, sym=bool(d["sym"]),
              eps=float(d["eps"]), threshold_method=str(d["method"]),
              actorder=bool(d["actorder"]), batch_size=int(d["batch"]), device=DEV)

    model = tiny(d)
    res = run_and_record(model, ids, str(tmp_path), evaluate_packed=lambda m: 1.0, pack=True,
                         clip_search=True, clip_grid=50, clip_steps=30, **kw)
    sd = model.state_dict()
    assert len(res["packed"]) == 14
    for name, t in res["packed"].items():
        back = dequantize_packed(t["qweight"], t["qzeros"], t["scales"], bits, group,
                                 torch.float32)
        assert torch.equal(back, sd[name + ".weight"]), name
    moved = 0
    for s in res["layer_stats"]:
        assert s["clip_j"] <= s["clip_j0"] and 0 <= s["clip_moved"] <= s["clip_groups"], s
        moved += s["clip_moved"]
    assert len(res["layer_stats"]) == 14 and moved > 0
    want = {"clip_search": True, "clip_grid": 50, "clip_steps": 30}
    rec = json.load(open(os.path.join(str(tmp_path), "results.json")))
    assert {k: rec["config"].get(k) for k in want} == want
    assert rec["layer_stats"][0]["clip_groups"] == res["layer_stats"][0]["clip_groups"]
    _, qc = read_quantized(os.path.join(str(tmp_path), "packed"))
    assert {k: qc["truncgptq"].get(k) for k in want} == want
    log = open(os.path.join(str(tmp_path), "quantization.log")).read()
    assert log.count("[Clip] weighted RTN error") == 14 and "groups clipped" in log

    plain, off = tiny(d), tiny(d)
    r_plain = quantize_model(plain, ids, **kw)
    r_off = quantize_model(off, ids, clip_search=False, **kw)
    for (k1, v1), (k2, v2) in zip(plain.state_dict().items(), off.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2), k1
    assert all("clip_j" not in s for s in r_plain["layer_stats"] + r_off["layer_stats"])
    assert any(not torch.equal(v, sd[k]) for k, v in plain.state_dict().items())
