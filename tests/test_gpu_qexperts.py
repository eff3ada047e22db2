"""Packed Mixture-of-Experts layers (A19) above the kernel: the QuantExperts
module, the checkpoint's "experts" entry and the solver loop's two experts
groups, on a tiny seeded Qwen3-MoE (2 layers, hidden 64, 4 experts of width 32,
top-2).  The router of every layer is cut to its first three rows, so expert 3
never receives a calibration row."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from qlinear_ref import packed_case

DEV = "cuda:0"
gpu = pytest.mark.gpu
E, H, I, K = 4, 64, 32, 2


def moe_config(**kw):
    from transformers import Qwen3MoeConfig
    cfg = Qwen3MoeConfig(vocab_size=128, hidden_size=H, intermediate_size=64,
                         moe_intermediate_size=I, num_hidden_layers=2, num_attention_heads=4,
                         num_key_value_heads=2, head_dim=16, num_experts=E, num_experts_per_tok=K,
                         decoder_sparse_step=1, mlp_only_layers=[], max_position_embeddings=64,
                         tie_word_embeddings=False, **kw)
    cfg._attn_implementation = "eager"
    return cfg


def tiny_moe():
    from transformers import Qwen3MoeForCausalLM
    torch.manual_seed(0)
    model = Qwen3MoeForCausalLM(moe_config()).float().eval()
    for layer in model.model.layers:
        layer.mlp.gate.weight = torch.nn.Parameter(layer.mlp.gate.weight[:E - 1].clone())
    ids = [torch.randint(0, 128, (1, 32), generator=torch.Generator().manual_seed(s))
           for s in range(6)]
    return model, ids


@gpu
def test_module_matches_the_recipe_and_the_float64_loop():
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeExperts
    from gptq_svd_amd.qlinear import QuantExperts, qgemm_grouped
    T = 19
    stacks = []
    for m, n in ((2 * I, H), (H, I)):
        cs = [packed_case(m, n, 32, 4, "small", seed=e) for e in range(E)]
        qw, qz, sc = (torch.from_numpy(np.stack([c[i] for c in cs])).to(DEV) for i in (3, 4, 5))
        stacks.append(dict(qweight=qw, qzeros=qz, scales=sc.half()))
    q = QuantExperts.from_packed(stacks[0], stacks[1], 4, 32)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(T, H, generator=gen).half().to(DEV)
    idx = torch.stack([torch.randperm(E - 1, generator=gen)[:K] for _ in range(T)]).to(DEV)
    w = torch.softmax(torch.randn(T, K, generator=gen), dim=-1).half().to(DEV)
    y = q(x, idx, w)
    assert y.shape == (T, H) and y.dtype == torch.float16 and "num_experts=4" in repr(q)

    # the three steps by hand
    flat = idx.reshape(-1)
    order = torch.argsort(flat, stable=True)
    off = torch.cat([flat.new_zeros(1), torch.bincount(flat, minlength=E).cumsum(0)]).int()
    gu = qgemm_grouped(x, (order // K).int(), off, q.gate_up_qweight, q.gate_up_qzeros,
                       q.gate_up_scales, 4, 32)
    d = qgemm_grouped(torch.nn.functional.silu(gu[:, :I]) * gu[:, I:], None, off, q.down_qweight,
                      q.down_qzeros, q.down_scales, 4, 32,
                      row_scale=w.reshape(-1)[order].float())
    d = d[torch.argsort(order)].view(T, K, H).float()
    assert torch.equal(y, (d[:, 0] + d[:, 1]).half())

    # float64 on the decoded weights, the HF loop's formula; HF's module in fp16
    Wg, Wd = q.dequantize(torch.float16)
    x64, w64, Wg64, Wd64 = (t.double().cpu() for t in (x, w, Wg, Wd))
    y64 = torch.zeros(T, H, dtype=torch.float64)
    for t in range(T):
        for j in range(K):
            e = int(idx[t, j])
            g, u = (x64[t] @ Wg64[e].T).chunk(2)
            y64[t] += w64[t, j] * ((torch.nn.functional.silu(g) * u) @ Wd64[e].T)
    hf = Qwen3MoeExperts(moe_config()).half().to(DEV)
    hf.gate_up_proj.data, hf.down_proj.data = Wg, Wd
    with torch.no_grad():
        e_hf = float((hf(x, idx, w).double().cpu() - y64).abs().max())
    e_q = float((y.double().cpu() - y64).abs().max())
    print(f"max err packed {e_q:.3e}, HF fp16 {e_hf:.3e}, ratio {e_q / e_hf:.3f}")
    assert e_q <= 2 * e_hf


@gpu
@pytest.mark.parametrize("fmt", ["int", "mxfp4"])
def test_moe_model_end_to_end(fmt, tmp_path):
    import gptq_svd_amd.gptq_utils as g
    from gptq_svd_amd.export import load_quantized, save_quantized
    from gptq_svd_amd.harness import quantize_model
    from gptq_svd_amd.qlinear import QuantExperts
    model, ids = tiny_moe()
    model = model.to(DEV)
    orig = copy.deepcopy(model.model.layers[0].mlp.experts.gate_up_proj.data)
    run = dict(mode="eigh", w_bits=4, group_size=32, eps=1e-2, batch_size=2, device=DEV)
    res = quantize_model(model, ids, pack=True, weight_format=fmt, **run)
    save_quantized(str(tmp_path), model, res["packed"], 4, 32, False, scale_dtype=torch.float32,
                   weight_format=fmt)
    names = [f"model.layers.{i}.mlp.experts" for i in range(2)]
    assert json.load(open(os.path.join(str(tmp_path), "quantize_config.json")))["experts"] == names
    packed = load_quantized(copy.deepcopy(model).half(), str(tmp_path), device=DEV).eval()

    # both modules come back packed and decode to the write-back; expert 3 had no rows
    for i, name in enumerate(names):
        qe, dense = packed.get_submodule(name), model.get_submodule(name)
        assert isinstance(qe, QuantExperts) and qe.weight_format == fmt
        Wg, Wd = qe.dequantize(torch.float32)
        assert torch.equal(Wg, dense.gate_up_proj.data) and torch.equal(Wd, dense.down_proj.data)
        for p in ("gate_up_proj", "down_proj"):
            entry, = [s for s in res["layer_stats"] if s["name"] == f"layer_{i}.mlp.experts.{p}"]
            assert entry["experts_without_rows"] == 1 and entry["experts"] == E
    if fmt == "int":    # H = I is round-to-nearest: within half a step of the original
        sc = res["packed"][names[0] + ".gate_up_proj"]["scales"][E - 1]      # (G, 2I)
        step = sc.t().repeat_interleave(32, dim=1)
        got = model.get_submodule(names[0]).gate_up_proj.data[E - 1]
        assert bool(((got - orig[E - 1]).abs() <= 0.5 * step * (1 + 1e-6)).all())

    # layer 0, every routed expert: the plain API on the rows the router sent it
    seen = []
    ex0 = model.get_submodule(names[0])
    h = ex0.register_forward_pre_hook(lambda mod, args: seen.append((args[0], args[1])))
    with torch.no_grad():
        for j in range(0, len(ids), 2):
            model(torch.cat(ids[j:j + 2]).to(DEV), use_cache=False)
    h.remove()
    for e in range(E - 1):
        acc = g.HessianAccumulator(H, DEV)
        for hs, idx in seen:
            acc.add_batch(hs[(idx == e).any(dim=-1)])
        assert acc.n_samples > 0
        R, R_x, perm = g.process_hessian_alt(acc.get_hessian(), 1e-2, "mean_trimmed")
        qz = g.Quantizer(4, 32, False, **({"weight_format": fmt} if fmt != "int" else {}))
        want, _ = g.gptq_fwrd(orig[e].float(), R, qz, perm, block_size=1024)
        assert torch.equal(ex0.gate_up_proj.data[e], want), f"expert {e}"

    # logits: dense fp32 write-back, the same in fp16, packed
    batch = torch.cat(ids[:4]).to(DEV)
    with torch.no_grad():
        L32 = model(batch).logits.float()
        L16 = copy.deepcopy(model).half()(batch).logits.float()
        Lq = packed(batch).logits.float()
    e16, eq = float((L16 - L32).abs().max()), float((Lq - L32).abs().max())
    print(f"{fmt}: max|Lq - L32| = {eq:.3e}, max|L16 - L32| = {e16:.3e}")
    assert eq <= 2 * e16, (eq, e16)
    if fmt == "mxfp4":
        with pytest.raises(ValueError, match="act_format"):
            load_quantized(copy.deepcopy(model).half(), str(tmp_path), act_format="mxfp8")


@gpu
def test_dense_model_has_no_experts_key(tmp_path):
    from transformers import Qwen3Config, Qwen3ForCausalLM
    from gptq_svd_amd.export import save_quantized
    from gptq_svd_amd.harness import quantize_model
    torch.manual_seed(0)
    cfg = Qwen3Config(vocab_size=128, hidden_size=H, intermediate_size=64, num_hidden_layers=1,
                      num_attention_heads=4, num_key_value_heads=2, head_dim=16)
    cfg._attn_implementation = "eager"
    model = Qwen3ForCausalLM(cfg).float().eval().to(DEV)
    res = quantize_model(model, tiny_moe()[1], mode="eigh", w_bits=4, group_size=32, batch_size=2,
                         device=DEV, pack=True)
    assert len(res["packed"]) == 7 and all(t["qweight"].dim() == 2 for t in res["packed"].values())
    save_quantized(str(tmp_path), model, res["packed"], 4, 32, False)
    assert "experts" not in json.load(open(os.path.join(str(tmp_path), "quantize_config.json")))


@gpu
@pytest.mark.parametrize("mode", ["svd", "gptq"])
def test_moe_model_other_modes(mode):
    """The sketch and plain-GPTQ branches of the experts solve, H = I for the
    expert without rows included: the packed stacks decode to the write-back."""
    from gptq_svd_amd.harness import quantize_model
    from gptq_svd_amd.qlinear import QuantExperts
    model, ids = tiny_moe()
    model = model.to(DEV)
    res = quantize_model(model, ids, mode=mode, pack=True, w_bits=4, group_size=32, batch_size=2,
                         device=DEV)
    for i in range(2):
        name = f"model.layers.{i}.mlp.experts"
        qe = QuantExperts.from_packed(res["packed"][name + ".gate_up_proj"],
                                      res["packed"][name + ".down_proj"], 4, 32)
        Wg, Wd = qe.dequantize(torch.float32)
        dense = model.get_submodule(name)
        assert torch.equal(Wg, dense.gate_up_proj.data) and torch.equal(Wd, dense.down_proj.data)
    assert [s["experts_without_rows"] for s in res["layer_stats"] if "experts" in s] == [1] * 4


@pytest.mark.parametrize("kw", [dict(lowrank=4), dict(rotate=32), dict(clip_search=True),
                                dict(world=2)])
def test_unsupported_combinations_raise_before_any_work(kw, monkeypatch):
    """No device is touched: the model is on the CPU and there is no calibration
    data.  world=2 stands for the multi-GPU harness mode (no process group is made)."""
    import gptq_svd_amd.harness as h
    kw = dict(kw)
    if kw.pop("world", None):
        monkeypatch.setattr(h, "_world", lambda pg=None: (2, 0))
    with pytest.raises(ValueError, match="Mixture-of-Experts"):
        h.quantize_model(tiny_moe()[0], [], **kw)


def test_shared_experts_raise_before_any_work():
    from transformers import Qwen2MoeConfig, Qwen2MoeForCausalLM
    from gptq_svd_amd.harness import quantize_model
    cfg = Qwen2MoeConfig(vocab_size=128, hidden_size=H, intermediate_size=64,
                         moe_intermediate_size=I, shared_expert_intermediate_size=I,
                         num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                         num_experts=E, num_experts_per_tok=K)
    with pytest.raises(ValueError, match="shared experts"):
        quantize_model(Qwen2MoeForCausalLM(cfg), [])
