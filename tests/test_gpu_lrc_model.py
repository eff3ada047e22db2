"""GPU: the low-rank correction end to end on the tiny random Qwen3 of the MX and
qlinear tests (2 layers, 14 linears): quantize_model(lowrank=8) ->
save_quantized -> load_quantized -> forward, in modes "eigh" and "svd", for the
integer grid (2 bits, groups of 32) and for MXFP4 (with and without MXFP8
activations); and the guards that lowrank=0 and checkpoints without the extra
tensors behave exactly as before.
"""
import copy
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 8


def tiny_model(d):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    cfg = Qwen3Config(**json.loads(str(d["config"])))
    cfg._attn_implementation = "eager"
    m = Qwen3ForCausalLM(cfg).float().eval()
    m.load_state_dict({k[len("init/"):]: torch.from_numpy(d[k]) for k in d
                       if k.startswith("init/")})
    return m


@pytest.fixture(scope="module")
def golden():
    return load_golden("h_qwen3tiny_eigh_w4a")


def calib(d):
    return [torch.from_numpy(r[None]) for r in d["ids"]]


def quantize(d, **kw):
    from gptq_svd_amd.harness import quantize_model
    model = tiny_model(d).to(DEV)
    args = dict(mode="eigh", eps=float(d["eps"]), threshold_method=str(d["method"]),
                batch_size=int(d["batch"]), device=DEV, pack=True)
    args.update(kw)
    return model, quantize_model(model, calib(d), **args)


def h_of(kw):
    """float64 H (host) from what the harness handed to lowrank_correction."""
    if kw.get("H") is not None:
        return kw["H"].double().cpu().numpy()
    F = kw["factor"].double().cpu().numpy()
    if kw.get("perm") is not None:
        Fg = np.empty_like(F)
        Fg[:, kw["perm"].cpu().numpy()] = F              # Fg[:, perm[j]] = F[:, j]
        F = Fg
    return F.T @ F


def logits_close(model, packed, d):
    """The closeness test_gpu_qlinear.py asks of QuantLinear: the packed logits
    are within twice the fp16-vs-fp32 distance of the dense write-back model."""
    dense16 = copy.deepcopy(model).half()
    batch = torch.cat(calib(d)[:4]).to(DEV)
    with torch.no_grad():
        L32 = model(batch).logits.float()
        L16 = dense16(batch).logits.float()
        Lq = packed(batch).logits.float()
    e16 = float((L16 - L32).abs().max())
    eq = float((Lq - L32).abs().max())
    print(f"[lrc model] max|Lq - L32| = {eq:.3e}, max|L16 - L32| = {e16:.3e}")
    assert torch.isfinite(Lq).all()
    assert eq <= 2 * e16, (eq, e16)


@pytest.mark.parametrize("mode", ["eigh", "svd"])
def test_quantize_save_load_forward(golden, tmp_path, monkeypatch, mode):
    from gptq_svd_amd import harness
    from gptq_svd_amd.export import load_quantized, read_quantized, save_quantized
    from gptq_svd_amd.qlinear import QuantLinear
    d = golden
    calls = []
    real = harness.lowrank_correction

    def spy(E, r, **kw):
        out = real(E, r, **kw)
        calls.append((E.double().cpu().numpy(), h_of(kw), out[2]))
        return out

    monkeypatch.setattr(harness, "lowrank_correction", spy)
    extra = dict(sketch_seed=7) if mode == "svd" else {}
    model, res = quantize(d, mode=mode, w_bits=2, group_size=32, lowrank=R, **extra)
    stats = res["layer_stats"]
    assert len(stats) == len(calls) == 14
    names = list(res["packed"])
    excess = 0.0
    for s, name, (E, H, info) in zip(stats, names, calls):
        assert 1 <= s["lr_rank"] <= R
        assert 0.0 <= s["lr_err1"] <= s["lr_err0"]
        assert s["lr_err0"] == info["err0"] and s["lr_err1"] == info["err1"]
        t = res["packed"][name]
        A, B = t["lr_a"], t["lr_b"]
        assert A.dtype == B.dtype == torch.float16
        assert A.shape == (E.shape[0], R) and B.shape == (R, E.shape[1])
        assert torch.isfinite(A).all() and torch.isfinite(B).all()
        D = E - A.double().cpu().numpy() @ B.double().cpu().numpy()
        err16 = float(np.sum((D @ H) * D))               # the stored fp16 factors, float64
        err0 = float(np.sum((E @ H) * E))
        assert abs(err0 - s["lr_err0"]) <= 1e-9 * err0
        excess = max(excess, (err16 - s["lr_err1"]) / s["lr_err0"])
        print(f"[lrc model] {mode} {s['name']}: err1 / err0 = {s['lr_err1'] / s['lr_err0']:.4f} "
              f"(fp16 factors {err16 / s['lr_err0']:.4f}), kept {s['lr_rank']}")
        assert err16 <= s["lr_err0"]
    print(f"[lrc model] {mode}: largest fp16-induced excess over err1, relative to err0: "
          f"{excess:.3e}")

    save_quantized(str(tmp_path), model, res["packed"], 2, 32, False,
                   scale_dtype=torch.float32)
    tensors, qc = read_quantized(str(tmp_path))
    assert qc["lowrank"] == R
    assert sum(k.endswith(".lr_a") for k in tensors) == 14
    packed = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV).eval()
    qmods = {n: m for n, m in packed.named_modules() if isinstance(m, QuantLinear)}
    assert len(qmods) == 14 and set(qmods) == set(res["packed"])
    sd = model.state_dict()
    for n, mod in qmods.items():
        assert mod.lr_a is not None and mod.lr_a.shape[1] == R and mod.lr_b.shape[0] == R
        # fp32 scales: the packed weight decodes to Wq exactly, and the effective
        # weight is the harness's write-back bit for bit (the same fma chain)
        assert torch.equal(mod.dequantize(torch.float32, effective=True), sd[n + ".weight"]), n
        eff16 = mod.dequantize(torch.float16, effective=True)
        assert torch.equal(eff16, sd[n + ".weight"].to(torch.float16)), n
        assert not torch.equal(mod.dequantize(torch.float32), sd[n + ".weight"]), n
    logits_close(model, packed, d)


@pytest.mark.parametrize("act_format", [None, "mxfp8"])
def test_mxfp4_with_lowrank(golden, tmp_path, act_format):
    from gptq_svd_amd.export import load_quantized, read_quantized, save_quantized
    from gptq_svd_amd.qlinear import MXQuantLinear
    d = golden
    model, res = quantize(d, weight_format="mxfp4", lowrank=R)
    for s in res["layer_stats"]:
        assert s["weight_format"] == "mxfp4" and 0.0 <= s["lr_err1"] <= s["lr_err0"]
    save_quantized(str(tmp_path), model, res["packed"], 4, 32, True, weight_format="mxfp4")
    tensors, qc = read_quantized(str(tmp_path))
    assert qc["checkpoint_format"] == "mxfp4" and qc["lowrank"] == R
    packed = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV,
                            act_format=act_format).eval()
    qmods = {n: m for n, m in packed.named_modules() if isinstance(m, MXQuantLinear)}
    assert len(qmods) == 14
    sd = model.state_dict()
    for n, mod in qmods.items():
        assert mod.act_format == act_format and mod.lr_a is not None
        assert torch.equal(mod.dequantize(torch.float32, effective=True), sd[n + ".weight"]), n
    if act_format is None:
        logits_close(model, packed, d)
        return
    # W4A8 has other numerics: measured against the weights-only packed model as
    # test_gpu_mxa.py does, within twice the distance of the torch emulation
    # (the same model with every linear's input passed through the MXFP8 image)
    from gptq_svd_amd.qlinear import dequantize_act_mx, quantize_act_mx
    plain = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV).eval()
    emul = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV).eval()

    def requantise(mod, args):
        x = args[0]
        return (dequantize_act_mx(*quantize_act_mx(x), x.dtype),)

    for mod in emul.modules():
        if isinstance(mod, MXQuantLinear):
            mod.register_forward_pre_hook(requantise)
    batch = torch.cat(calib(d)[:4]).to(DEV)
    with torch.no_grad():
        Lw = plain(batch).logits.float()
        La = packed(batch).logits.float()
        Le = emul(batch).logits.float()
    assert torch.isfinite(La).all() and not torch.equal(La, Lw)
    rel_a = float((La - Lw).norm() / Lw.norm())
    rel_e = float((Le - Lw).norm() / Lw.norm())
    print(f"[lrc model] mxfp4 + mxfp8: |La - Lw| / |Lw| = {rel_a:.3e}, emulated {rel_e:.3e}")
    assert rel_a <= 2 * rel_e, (rel_a, rel_e)


def test_lowrank_zero_is_todays_run(golden):
    d = golden
    m0, r0 = quantize(d, w_bits=4, group_size=32)
    m1, r1 = quantize(d, w_bits=4, group_size=32, lowrank=0)
    assert set(r0["packed"]) == set(r1["packed"])
    for n, t in r0["packed"].items():
        assert set(t) == set(r1["packed"][n]) == {"qweight", "qzeros", "scales"}
        for k in t:
            assert torch.equal(t[k], r1["packed"][n][k]), (n, k)
    for (k0, v0), (k1, v1) in zip(m0.state_dict().items(), m1.state_dict().items()):
        assert k0 == k1 and torch.equal(v0, v1), k0
    assert all("lr_rank" not in s for s in r1["layer_stats"])


def test_checkpoint_without_lowrank_loads_as_before(golden, tmp_path):
    from gptq_svd_amd.export import load_quantized, read_quantized, save_quantized
    from gptq_svd_amd.qlinear import QuantLinear
    d = golden
    model, res = quantize(d, w_bits=4, group_size=32)
    save_quantized(str(tmp_path), model, res["packed"], 4, 32, False)
    tensors, qc = read_quantized(str(tmp_path))
    assert "lowrank" not in qc and not any(".lr_" in k for k in tensors)
    packed = load_quantized(tiny_model(d).half(), str(tmp_path), device=DEV).eval()
    mods = [m for m in packed.modules() if isinstance(m, QuantLinear)]
    assert len(mods) == 14
    for m in mods:
        assert m.lr_a is None and m.lr_b is None
        assert not {"lr_a", "lr_b"} & set(m.state_dict())
        assert torch.equal(m.dequantize(torch.float16, effective=True), m.dequantize())
    logits_close(model, packed, d)
    # half a pair is refused
    from safetensors.torch import save_file
    name = next(k[:-len(".qweight")] for k in tensors if k.endswith(".qweight"))
    n_in = tensors[name + ".g_idx"].numel()
    save_file(dict(tensors, **{name + ".lr_b": torch.zeros(4, n_in, dtype=torch.float16)}),
              str(tmp_path / "model.safetensors"), metadata={"format": "pt"})
    with pytest.raises(KeyError, match="lr_a and lr_b"):
        load_quantized(tiny_model(d).half(), str(tmp_path))


def test_lowrank_with_clip_search(golden):
    d = golden
    _, res = quantize(d, w_bits=3, group_size=32, lowrank=4, clip_search=True, pack=False)
    for s in res["layer_stats"]:
        assert "clip_j" in s and 0.0 <= s["lr_err1"] <= s["lr_err0"] and s["lr_rank"] >= 1
    assert res["packed"] == {}


def test_gptq_mode_uses_the_hessian(golden):
    d = golden
    _, res = quantize(d, mode="gptq", w_bits=3, group_size=32, lowrank=4, pack=False)
    for s in res["layer_stats"]:
        assert 0.0 <= s["lr_err1"] <= s["lr_err0"] and s["lr_rank"] >= 1


def test_lowrank_refuses_the_multi_gpu_mode(monkeypatch):
    from gptq_svd_amd import harness as h
    monkeypatch.setattr(h, "_world", lambda pg=None: (2, 0))
    with pytest.raises(ValueError, match="lowrank is single-process"):
        h.quantize_model(None, [], lowrank=8)
