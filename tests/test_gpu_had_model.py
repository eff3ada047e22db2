"""GPU: the Hadamard rotation end to end on the tiny random Qwen3 of the model
tests (hidden 128, intermediate 256: the automatic block is 128 or 256; 2 layers,
14 linears): quantize_model(rotate=-1) -> save_quantized -> load_quantized ->
forward, for the integer grid (4 bits, groups of 32) and MXFP4 (with and without
MXFP8 activations), with and without the low-rank correction; and the guards
that rotate=0 and checkpoints without the key behave exactly as before.

Per module the forward is held to
  |y - x W^T| <= 2 n 2^-24 |x'| |W'|^T + ulp16(y) + u16 |x'| |W'|^T
with W = dequantize(float32, rotated=False), x' = x Q rounded to 16 bits and W'
the stored-basis weight: the fp32 GEMM bound of test_gpu_qlinear.py on (x', W')
plus the 16-bit rounding of x' (u16 = 2^-11 for fp16).  With a low-rank
correction the same two terms are added for the second product,
2 (n + r) 2^-24 + u16 times (|x'| |B|^T) |A|^T (test_gpu_lrinfer.py's term).
The MXFP8-activation variant has other numerics (x' is quantised to e4m3) and is
held to the emulation criterion of test_gpu_lrc_model.py instead.
Worst err / bound measured on an MI355X: DESIGN.md "Hadamard rotation".
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_lrc_model import calib, logits_close, tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U16 = 2.0 ** -11
WORST = {"ratio": 0.0}

VARIANTS = {
    "int4g32": (dict(w_bits=4, group_size=32), None),
    "mxfp4": (dict(weight_format="mxfp4"), None),
    "mxfp4_mxfp8": (dict(weight_format="mxfp4"), "mxfp8"),
    "int4g32_lr8": (dict(w_bits=4, group_size=32, lowrank=8), None),
    "mxfp4_lr8": (dict(weight_format="mxfp4", lowrank=8), None),
    "mxfp4_mxfp8_lr8": (dict(weight_format="mxfp4", lowrank=8), "mxfp8"),
}


@pytest.fixture(scope="module")
def golden():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return load_golden("h_qwen3tiny_eigh_w4a")


def quantize(d, **kw):
    from gptq_svd_amd.harness import quantize_model
    model = tiny_model(d).to(DEV)
    args = dict(mode="eigh", eps=float(d["eps"]), threshold_method=str(d["method"]),
                batch_size=int(d["batch"]), device=DEV, pack=True)
    args.update(kw)
    return model, quantize_model(model, calib(d), **args)


def save(path, model, res, qkw):
    from gptq_svd_amd.export import save_quantized
    if qkw.get("weight_format") == "mxfp4":
        save_quantized(path, model, res["packed"], 4, 32, True, weight_format="mxfp4")
    else:
        save_quantized(path, model, res["packed"], qkw["w_bits"], qkw["group_size"], False,
                       scale_dtype=torch.float32)


def ulp16(y64):
    e = np.floor(np.log2(np.maximum(np.abs(y64), 1e-300)))
    return 2.0 ** (np.maximum(e, -14) - 10)


def unrotated_twin(mod):
    """The same packed tensors in a module that does not rotate."""
    from gptq_svd_amd.qlinear import MXQuantLinear
    lr = (mod.lr_a, mod.lr_b) if mod.lr_a is not None else None
    if isinstance(mod, MXQuantLinear):
        return type(mod).from_packed(mod.qweight, mod.scales, bias=mod.bias,
                                     act_format=mod.act_format, lowrank=lr)
    return type(mod).from_packed(mod.qweight, mod.qzeros, mod.scales, mod.w_bits, mod.group_size,
                                 bias=mod.bias, lowrank=lr)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_quantize_save_load_forward(golden, tmp_path, variant):
    from gptq_svd_amd.export import load_quantized, read_quantized
    from gptq_svd_amd.gptq_utils import HadamardRotation
    from gptq_svd_amd.harness import _rotation_seed
    from gptq_svd_amd.qlinear import MXQuantLinear, QuantLinear, hadamard
    d = golden
    qkw, act = VARIANTS[variant]
    model, res = quantize(d, rotate=-1, rotate_seed=3, **qkw)
    assert len(res["layer_stats"]) == 14
    for s in res["layer_stats"]:
        want = 256 if s["name"].endswith("down_proj") else 128
        assert s["rotate_block"] == want, s
    for name, t in res["packed"].items():
        assert t["had_block"] in (128, 256) and t["had_sign"].dtype == torch.int32
    # the documented seed: (rotate_seed, layer, group)
    t = res["packed"]["model.layers.1.mlp.down_proj"]
    assert torch.equal(t["had_sign"].cpu(),
                       HadamardRotation(256, 256, seed=_rotation_seed(3, 1, 3),
                                        device="cpu").sign_bits)
    save(str(tmp_path), model, res, qkw)
    tensors, qc = read_quantized(str(tmp_path))
    assert qc["rotation"]["kind"] == "hadamard" and len(qc["rotation"]["blocks"]) == 14
    assert sum(k.endswith(".had_sign") for k in tensors) == 14
    akw = dict(act_format=act) if act else {}
    packed = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV, **akw).eval()
    cls = MXQuantLinear if qkw.get("weight_format") == "mxfp4" else QuantLinear
    qmods = {n: m for n, m in packed.named_modules() if isinstance(m, cls)}
    assert len(qmods) == 14 and set(qmods) == set(res["packed"])
    sd = model.state_dict()
    gen = torch.Generator().manual_seed(0)
    for n, mod in qmods.items():
        blk = 256 if n.endswith("down_proj") else 128
        assert mod.rotate_block == blk == qc["rotation"]["blocks"][n]
        assert mod.had_sign is not None and mod.had_sign.numel() == mod.in_features // 32
        assert torch.equal(mod.had_sign, res["packed"][n]["had_sign"])
        # the write-back is R^-1 of the stored weight (+ the rotated-back correction)
        eff = mod.dequantize(torch.float32, effective=True, rotated=False)
        if mod.lr_a is None:
            assert torch.equal(eff, sd[n + ".weight"]), n
        else:
            # (Wq' + A B) Q^T here, Wq' Q^T + A (B Q^T) in the harness: two orders of the
            # same sums, each log2 b + r + 3 fp32 roundings on terms whose absolute
            # sum is at most sqrt(b) max|W'|
            r, Wp = mod.lr_a.shape[1], mod.dequantize(torch.float32, effective=True)
            tol = 2 * (np.log2(blk) + r + 3) * 2.0 ** -24 * np.sqrt(blk) * float(Wp.abs().max())
            assert float((eff - sd[n + ".weight"]).abs().max()) <= tol, n
        assert not torch.equal(mod.dequantize(torch.float32), eff)
        # forward = hadamard, then the unrotated module on x', bit for bit
        x = (torch.randn(5, mod.in_features, generator=gen) * 2).half().to(DEV)
        y = mod(x)
        xr = hadamard(x, mod.rotate_block, mod.had_sign)
        assert xr.dtype == torch.float16
        assert torch.equal(y, unrotated_twin(mod)(xr)), n
        if act is not None:
            continue
        # the derived bound against the original-basis weight
        W = eff.double().cpu().numpy()
        Ws = mod.dequantize(torch.float32).double().cpu().numpy()
        x64, xr64 = x.double().cpu().numpy(), xr.double().cpu().numpy()
        y64 = x64 @ W.T
        nn = mod.in_features
        prod = np.abs(xr64) @ np.abs(Ws).T
        bound = 2 * nn * 2.0 ** -24 * prod + ulp16(y64) + U16 * prod
        if mod.lr_a is not None:
            A, B = mod.lr_a.double().cpu().numpy(), mod.lr_b.double().cpu().numpy()
            lr = (np.abs(xr64) @ np.abs(B).T) @ np.abs(A).T
            bound = bound + (2 * (nn + A.shape[1]) * 2.0 ** -24 + U16) * lr
        err = np.abs(y.double().cpu().numpy() - y64)
        ratio = float((err / bound).max())
        WORST["ratio"] = max(WORST["ratio"], ratio)
        assert ratio <= 1.0, (n, ratio)
    print(f"[had model] {variant}: worst err / bound {WORST['ratio']:.3f} so far")
    if act is None:
        logits_close(model, packed, d)
        return
    # W4A8: against the weights-only packed model, within twice the distance of the
    # torch emulation (every linear's rotated input passed through the MXFP8 image)
    from gptq_svd_amd.qlinear import dequantize_act_mx, quantize_act_mx
    plain = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV).eval()
    emul = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV).eval()
    for mod in emul.modules():
        if isinstance(mod, MXQuantLinear):
            twin = unrotated_twin(mod)
            blk, sign = mod.rotate_block, mod.had_sign

            def fwd(x, twin=twin, blk=blk, sign=sign):
                xr = hadamard(x, blk, sign)
                return twin(dequantize_act_mx(*quantize_act_mx(xr), x.dtype))
            mod.forward = fwd
    batch = torch.cat(calib(d)[:4]).to(DEV)
    with torch.no_grad():
        Lw = plain(batch).logits.float()
        La = packed(batch).logits.float()
        Le = emul(batch).logits.float()
    assert torch.isfinite(La).all() and not torch.equal(La, Lw)
    rel_a = float((La - Lw).norm() / Lw.norm())
    rel_e = float((Le - Lw).norm() / Lw.norm())
    print(f"[had model] {variant}: |La - Lw| / |Lw| = {rel_a:.3e}, emulated {rel_e:.3e}")
    assert rel_a <= 2 * rel_e, (rel_a, rel_e)


def test_rotate_zero_is_todays_run(golden, tmp_path):
    d = golden
    m0, r0 = quantize(d, w_bits=4, group_size=32, save_path=str(tmp_path / "a"))
    m1, r1 = quantize(d, w_bits=4, group_size=32, rotate=0, rotate_seed=9,
                      save_path=str(tmp_path / "b"))
    assert set(r0["packed"]) == set(r1["packed"])
    for n, t in r0["packed"].items():
        assert set(t) == set(r1["packed"][n]) == {"qweight", "qzeros", "scales"}
        for k in t:
            assert torch.equal(t[k], r1["packed"][n][k]), (n, k)
    for (k0, v0), (k1, v1) in zip(m0.state_dict().items(), m1.state_dict().items()):
        assert k0 == k1 and torch.equal(v0, v1), k0
    assert all("rotate_block" not in s for s in r1["layer_stats"])
    j0 = json.load(open(os.path.join(str(tmp_path / "a"), "results.json")))
    j1 = json.load(open(os.path.join(str(tmp_path / "b"), "results.json")))
    assert "rotate" not in j1["config"] and "rotate_seed" not in j1["config"]
    c0 = {k: v for k, v in j0["config"].items() if k != "save_path"}
    c1 = {k: v for k, v in j1["config"].items() if k != "save_path"}
    assert c0 == c1 and list(j0) == list(j1)
    strip = [{k: v for k, v in s.items() if k != "time"} for s in j0["layer_stats"]]
    assert strip == [{k: v for k, v in s.items() if k != "time"} for s in j1["layer_stats"]]
    # and with rotation on the config block records both fields
    _, _ = quantize(d, w_bits=4, group_size=32, rotate=128, rotate_seed=9,
                    save_path=str(tmp_path / "c"))
    j2 = json.load(open(os.path.join(str(tmp_path / "c"), "results.json")))
    assert j2["config"]["rotate"] == 128 and j2["config"]["rotate_seed"] == 9
    assert all(s["rotate_block"] == 128 for s in j2["layer_stats"])


def test_checkpoint_without_rotation_loads_as_before(golden, tmp_path):
    from gptq_svd_amd.export import load_quantized, read_quantized, save_quantized
    from gptq_svd_amd.qlinear import QuantLinear
    d = golden
    model, res = quantize(d, w_bits=4, group_size=32)
    save_quantized(str(tmp_path), model, res["packed"], 4, 32, False)
    tensors, qc = read_quantized(str(tmp_path))
    assert "rotation" not in qc and not any(k.endswith("had_sign") for k in tensors)
    packed = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV).eval()
    mods = [m for m in packed.modules() if isinstance(m, QuantLinear)]
    assert len(mods) == 14
    for m in mods:
        assert m.rotate_block == 0 and m.had_sign is None and "had_sign" not in m.state_dict()
        assert torch.equal(m.dequantize(torch.float16, rotated=False), m.dequantize())
    logits_close(model, packed, d)


@pytest.mark.parametrize("mode", ["svd", "gptq"])
def test_other_modes_with_clip_search(golden, mode):
    d = golden
    extra = dict(sketch_seed=7) if mode == "svd" else {}
    _, res = quantize(d, mode=mode, w_bits=3, group_size=32, rotate=-1, clip_search=True,
                      lowrank=4, pack=False, **extra)
    for s in res["layer_stats"]:
        assert s["rotate_block"] in (128, 256) and "clip_j" in s
        assert 0.0 <= s["lr_err1"] <= s["lr_err0"]
    assert res["packed"] == {}


def test_bad_blocks_raise_before_any_work(monkeypatch):
    from gptq_svd_amd import harness as h
    d = load_golden("h_qwen3tiny_eigh_w4a")
    model = tiny_model(d)                       # on the CPU: nothing may run

    def boom(*a, **k):
        raise AssertionError("work started")

    monkeypatch.setattr(h, "capture_initial_inputs", boom)
    for bad in (96, 48, 16, 8192):
        with pytest.raises(ValueError, match="rotate"):
            h.quantize_model(model, calib(d), rotate=bad)
    with pytest.raises(ValueError, match="does not divide"):
        h.quantize_model(model, calib(d), rotate=256)          # hidden = 128
    # a 96-wide linear: 64 does not divide it, and the automatic block is 32
    lin = model.model.layers[1].self_attn.o_proj
    wide = torch.nn.Linear(96, lin.out_features, bias=False)
    model.model.layers[1].self_attn.o_proj = wide
    with pytest.raises(ValueError, match="does not divide in_features=96"):
        h.quantize_model(model, calib(d), rotate=64)
    monkeypatch.setattr(h, "_world", lambda pg=None: (2, 0))
    with pytest.raises(ValueError, match="rotate is single-process"):
        h.quantize_model(None, [], rotate=-1)
