"""Packed checkpoint exporter (§8(f) rank 2; A13 -- the reference saves only
dequantised FP16 weights, quantize.py:262-273, README.md:133).

Layout (AutoGPTQ / GPTQModel "gptq_v2" checkpoint format, static groups):
for every quantised linear ``<name>``
  ``<name>.qweight`` int32 (in*b/32, out)  codes packed along in_features,
  ``<name>.qzeros``  int32 (G, out*b/32)   zero points packed along out_features
                                           (true zeros: v2, not the v1 "zero - 1"),
  ``<name>.scales``  fp16  (G, out)        (or fp32 with scale_dtype=torch.float32),
  ``<name>.g_idx``   int32 (in,)           = column // group_size (static groups
                                           in the original column order, so it
                                           is only the trivial map),
  ``<name>.bias``    as in the model;
every other tensor of the state dict as is.  ``quantize_config.json`` records
bits / group_size / sym / desc_act=false / static_groups=true and the
TruncGPTQ settings and per-layer ranks.  Dequantisation:
W[:, j] = (code_u[:, j] - zero_u[:, g(j)]) * scale[:, g(j)], with symmetric
codes stored +2^(b-1) (so zero_u = 2^(b-1)).

MXFP4 (``weight_format="mxfp4"``; ``"checkpoint_format": "mxfp4"``, bits 4,
group_size 32): per linear only
  ``<name>.qweight`` int32 (in/8, out)    E2M1 codes, the same 4-bit stream,
  ``<name>.scales``  uint8 (in/32, out)   E8M0 bytes, scale = 2^(byte - 127),
and the bias; W[:, j] = +-{0, .5, 1, 1.5, 2, 3, 4, 6}[code & 7] * scale[:, j // 32],
the sign in bit 3 of the code.

Low-rank correction (``quantize_model(lowrank=r)``): a corrected linear also has
  ``<name>.lr_a`` (out, r) and ``<name>.lr_b`` (r, in), fp16 / bf16 / fp32,
its effective weight being W + lr_a lr_b, and ``quantize_config.json`` records
``"lowrank": r``.  Checkpoints without these tensors are read exactly as before.
Loaders that do not know the two tensors (AutoGPTQ, GPTQModel) cannot apply
the correction.

Hadamard rotation (``quantize_model(rotate=...)``): a rotated linear also has
  ``<name>.had_sign`` int32 (in/32,), bit j of word i = input column 32 i + j is
  negated, and ``quantize_config.json`` records ``"rotation": {"kind":
  "hadamard", "blocks": {name: block}}``.  Its packed weight (and ``lr_b``) is
  that of the rotated basis W Q, so a consumer must apply x -> x Q to the
  layer's input.  Checkpoints without the key are read exactly
  as before.

``load_quantized`` is the way back: it puts the packed tensors into
``qlinear.QuantLinear`` (``qlinear.MXQuantLinear`` for MXFP4) modules of a
model, which run them without unpacking.
"""
from __future__ import annotations

import json
import os
from typing import Any, Dict, Optional

import torch

__all__ = ["save_quantized", "read_quantized", "load_quantized"]


def save_quantized(path: str, model: torch.nn.Module, packed: Dict[str, Dict[str, torch.Tensor]],
                   w_bits: int, group_size: int, sym: bool,
                   extra_config: Optional[Dict[str, Any]] = None,
                   scale_dtype: torch.dtype = torch.float16,
                   weight_format: str = "int") -> str:
    """Write ``model.safetensors`` + ``quantize_config.json`` (+ ``config.json``
    when the model has a HF config) into `path`; returns the tensor file path.
    ``weight_format="mxfp4"``: `packed` holds ``pack_quantized``'s MXFP4 pairs
    (``qzeros`` None); `w_bits` must be 4 and `group_size` 32, `sym` and
    `scale_dtype` are not used."""
    from safetensors.torch import save_file
    if weight_format not in ("int", "mxfp4"):
        raise ValueError(f"weight_format must be 'int' or 'mxfp4', got {weight_format!r}")
    mx = weight_format == "mxfp4"
    if mx and (int(w_bits) != 4 or int(group_size) != 32):
        raise ValueError(f"weight_format='mxfp4' needs w_bits=4 and group_size=32, got "
                         f"w_bits={w_bits}, group_size={group_size}")
    os.makedirs(path, exist_ok=True)
    sd = model.state_dict()
    tensors: Dict[str, torch.Tensor] = {}
    lowrank = 0
    blocks: Dict[str, int] = {}
    for name, t in packed.items():
        if (t.get("had_sign") is None) != (not t.get("had_block")):
            raise ValueError(f"{name}: had_sign and had_block come together")
        if t.get("had_sign") is not None:
            if t["had_sign"].dtype != torch.int32:
                raise ValueError(f"{name}: had_sign must be int32, got {t['had_sign'].dtype}")
            tensors[f"{name}.had_sign"] = t["had_sign"].contiguous().cpu()
            blocks[name] = int(t["had_block"])
        if (t.get("lr_a") is None) != (t.get("lr_b") is None):
            raise ValueError(f"{name}: lr_a and lr_b come together")
        if t.get("lr_a") is not None:
            tensors[f"{name}.lr_a"] = t["lr_a"].contiguous().cpu()
            tensors[f"{name}.lr_b"] = t["lr_b"].contiguous().cpu()
            lowrank = max(lowrank, int(t["lr_a"].shape[1]))
        if mx:
            if t["scales"].dtype != torch.uint8:
                raise ValueError(f"{name}: MXFP4 scales must be uint8, got {t['scales'].dtype}")
            tensors[f"{name}.qweight"] = t["qweight"].contiguous().cpu()
            tensors[f"{name}.scales"] = t["scales"].contiguous().cpu()
            continue
        in_features = t["qweight"].shape[0] * 32 // w_bits
        g = group_size if group_size > 0 else in_features
        tensors[f"{name}.qweight"] = t["qweight"].contiguous().cpu()
        tensors[f"{name}.qzeros"] = t["qzeros"].contiguous().cpu()
        tensors[f"{name}.scales"] = t["scales"].to(scale_dtype).contiguous().cpu()
        tensors[f"{name}.g_idx"] = (torch.arange(in_features, dtype=torch.int32) // g)
    for k, v in sd.items():
        mod = k.rsplit(".", 1)[0]
        if mod in packed and k.endswith(".weight"):
            continue  # replaced by the packed tensors
        tensors[k] = v.detach().contiguous().cpu()
    # tied parameters share storage: safetensors refuses aliases, so clone
    seen = {}
    for k in list(tensors):
        key = (tensors[k].untyped_storage().data_ptr(), tensors[k].storage_offset())
        if key in seen:
            tensors[k] = tensors[k].clone()
        seen[key] = k
    fn = os.path.join(path, "model.safetensors")
    save_file(tensors, fn, metadata={"format": "pt"})
    qc = {"bits": int(w_bits), "group_size": int(group_size), "sym": bool(sym),
          "desc_act": False, "static_groups": True, "true_sequential": True,
          "quant_method": "gptq", "checkpoint_format": "gptq_v2",
          "scale_dtype": str(scale_dtype).replace("torch.", "")}
    if mx:
        qc.update(sym=True, checkpoint_format="mxfp4", scale_dtype="e8m0")
    if lowrank:
        qc["lowrank"] = lowrank
    if blocks:
        qc["rotation"] = {"kind": "hadamard", "blocks": blocks}
    if extra_config:
        qc["truncgptq"] = extra_config
    with open(os.path.join(path, "quantize_config.json"), "w") as f:
        json.dump(qc, f, indent=2)
    cfg = getattr(model, "config", None)
    if cfg is not None and hasattr(cfg, "save_pretrained"):
        cfg.save_pretrained(path)
    return fn


def read_quantized(path: str):
    """(tensors dict, quantize_config dict) of a checkpoint written by
    save_quantized (plain reads; the consumer is load_quantized / qlinear)."""
    from safetensors.torch import load_file
    tensors = load_file(os.path.join(path, "model.safetensors"))
    with open(os.path.join(path, "quantize_config.json")) as f:
        qc = json.load(f)
    return tensors, qc


def _lowrank_of(tensors: Dict[str, torch.Tensor], name: str, keys: Dict[str, str]):
    """The (lr_a, lr_b) pair of a linear, or None; `keys` gains their names."""
    keys.update(lr_a=f"{name}.lr_a", lr_b=f"{name}.lr_b")
    a, b = tensors.get(keys["lr_a"]), tensors.get(keys["lr_b"])
    if (a is None) != (b is None):
        raise KeyError(f"{name}: lr_a and lr_b come together, the checkpoint holds one")
    return None if a is None else (a, b)


def _rotation_blocks(qc: Dict[str, Any], tensors: Dict[str, torch.Tensor]) -> Dict[str, int]:
    """{name: block} of the checkpoint's "rotation" entry ({} without one),
    checked against the ``had_sign`` tensors it holds."""
    rot = qc.get("rotation")
    if rot is None:
        blocks = {}
    elif not isinstance(rot, dict) or rot.get("kind") != "hadamard" \
            or not isinstance(rot.get("blocks"), dict):
        raise ValueError(f"quantize_config.json: unsupported rotation entry {rot!r}")
    else:
        blocks = {k: int(v) for k, v in rot["blocks"].items()}
    signed = {k[:-len(".had_sign")] for k in tensors if k.endswith(".had_sign")}
    if signed != set(blocks):
        raise KeyError(f"quantize_config.json's rotation blocks and the had_sign tensors "
                       f"disagree: {sorted(signed ^ set(blocks))}")
    return blocks


def _rotation_of(tensors: Dict[str, torch.Tensor], name: str, blocks: Dict[str, int],
                 keys: Dict[str, str]):
    """The (block, sign_bits) pair of a linear, or None; `keys` gains the tensor's name."""
    keys.update(had_sign=f"{name}.had_sign")
    return (blocks[name], tensors[keys["had_sign"]]) if name in blocks else None


def _set_submodule(model: torch.nn.Module, name: str, new: torch.nn.Module) -> None:
    parent_name, _, leaf = name.rpartition(".")
    parent = model.get_submodule(parent_name) if parent_name else model
    setattr(parent, leaf, new)


def load_quantized(model: torch.nn.Module, path: str, device=None,
                   act_format=None) -> torch.nn.Module:
    """Load a checkpoint written by save_quantized into `model` (the dense
    architecture, any weights) and return it: every ``nn.Linear`` whose
    ``<name>.qweight`` is in the checkpoint becomes a ``qlinear.QuantLinear``
    holding the packed tensors (bias kept, in the linear's dtype); every other
    tensor is loaded as is.  A linear with ``<name>.lr_a`` / ``<name>.lr_b`` gets
    them as its low-rank correction, and one listed in the ``"rotation"`` entry its
    ``had_sign`` and block (the module then rotates its input).
    ``quantize_config.json`` must be a static-group
    ``desc_act=false`` configuration with supported bits, and every ``g_idx``
    must be the trivial ``arange(in) // group`` map (act-order checkpoints are
    out of scope).  `device`: where the model is moved (default: it stays).
    `act_format`: a run-time choice for MXFP4 checkpoints, handed to every
    ``MXQuantLinear`` (None: 16-bit activations; "mxfp8": the block-scaled W4A8
    kernel); with an integer checkpoint it is an error.  The checkpoint does not
    record it."""
    from .qlinear import QuantLinear, _check_act_format
    _check_act_format(act_format)
    if act_format is not None:                   # before any tensor is read
        with open(os.path.join(path, "quantize_config.json")) as f:
            fmt = json.load(f).get("checkpoint_format", "gptq_v2")
        if fmt != "mxfp4":
            raise ValueError(f"act_format={act_format!r} needs an mxfp4 checkpoint; this one is "
                             f"{fmt!r}")
    tensors, qc = read_quantized(path)
    bits, group = int(qc["bits"]), int(qc["group_size"])
    blocks = _rotation_blocks(qc, tensors)
    if qc.get("checkpoint_format") == "mxfp4":
        return _load_mx(model, tensors, qc, device, act_format, blocks)
    if bits not in (2, 3, 4, 8):
        raise ValueError(f"quantize_config.json: bits={bits} is not one of 2, 3, 4, 8")
    if qc.get("desc_act", False):
        raise ValueError("quantize_config.json: desc_act=true (act-order) checkpoints are not "
                         "supported")
    if not isinstance(qc.get("sym"), bool):
        raise ValueError("quantize_config.json: sym must be true or false")
    fmt = qc.get("checkpoint_format", "gptq_v2")
    if fmt != "gptq_v2":
        raise ValueError(f"quantize_config.json: checkpoint_format={fmt!r}; only gptq_v2 (true "
                         "zero points) and mxfp4 are supported")
    names = [k[:-len(".qweight")] for k in tensors if k.endswith(".qweight")]
    used = set()
    for name in names:
        try:
            lin = model.get_submodule(name)
        except AttributeError:
            raise KeyError(f"{name}: packed in the checkpoint but absent from the model") from None
        if not isinstance(lin, torch.nn.Linear):
            raise TypeError(f"{name}: expected nn.Linear, found {type(lin).__name__}")
        keys = {k: f"{name}.{k}" for k in ("qweight", "qzeros", "scales", "g_idx", "bias")}
        for k in ("qzeros", "scales", "g_idx"):
            if keys[k] not in tensors:
                raise KeyError(f"{keys[k]} is missing from the checkpoint")
        bias = tensors.get(keys["bias"])
        if (bias is None) != (lin.bias is None):
            raise ValueError(f"{name}: the checkpoint and the model disagree about a bias")
        if bias is not None:
            bias = bias.to(lin.bias.dtype)
        lowrank = _lowrank_of(tensors, name, keys)
        rotation = _rotation_of(tensors, name, blocks, keys)
        try:
            q = QuantLinear.from_packed(tensors[keys["qweight"]], tensors[keys["qzeros"]],
                                        tensors[keys["scales"]], bits, group, bias=bias,
                                        g_idx=tensors[keys["g_idx"]], device=lin.weight.device,
                                        lowrank=lowrank, rotation=rotation)
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
        if (q.out_features, q.in_features) != (lin.out_features, lin.in_features):
            raise ValueError(f"{name}: packed weight is {q.out_features} x {q.in_features}, the "
                             f"model's linear is {lin.out_features} x {lin.in_features}")
        _set_submodule(model, name, q)
        used.update(v for v in keys.values() if v in tensors)
    return _load_rest(model, tensors, used, device)


def _load_mx(model: torch.nn.Module, tensors: Dict[str, torch.Tensor], qc: Dict[str, Any],
             device, act_format=None, blocks=None) -> torch.nn.Module:
    """load_quantized for ``checkpoint_format: "mxfp4"``: every ``nn.Linear``
    with a ``<name>.qweight`` becomes a ``qlinear.MXQuantLinear``."""
    from .qlinear import MXQuantLinear
    if int(qc["bits"]) != 4 or int(qc["group_size"]) != 32:
        raise ValueError(f"quantize_config.json: mxfp4 needs bits=4 and group_size=32, got "
                         f"bits={qc['bits']}, group_size={qc['group_size']}")
    if qc.get("desc_act", False):
        raise ValueError("quantize_config.json: desc_act=true (act-order) checkpoints are not "
                         "supported")
    used = set()
    for name in [k[:-len(".qweight")] for k in tensors if k.endswith(".qweight")]:
        try:
            lin = model.get_submodule(name)
        except AttributeError:
            raise KeyError(f"{name}: packed in the checkpoint but absent from the model") from None
        if not isinstance(lin, torch.nn.Linear):
            raise TypeError(f"{name}: expected nn.Linear, found {type(lin).__name__}")
        keys = {k: f"{name}.{k}" for k in ("qweight", "scales", "bias")}
        if keys["scales"] not in tensors:
            raise KeyError(f"{keys['scales']} is missing from the checkpoint")
        bias = tensors.get(keys["bias"])
        if (bias is None) != (lin.bias is None):
            raise ValueError(f"{name}: the checkpoint and the model disagree about a bias")
        if bias is not None:
            bias = bias.to(lin.bias.dtype)
        lowrank = _lowrank_of(tensors, name, keys)
        rotation = _rotation_of(tensors, name, blocks or {}, keys)
        try:
            q = MXQuantLinear.from_packed(tensors[keys["qweight"]], tensors[keys["scales"]],
                                          bias=bias, device=lin.weight.device,
                                          act_format=act_format, lowrank=lowrank,
                                          rotation=rotation)
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
        if (q.out_features, q.in_features) != (lin.out_features, lin.in_features):
            raise ValueError(f"{name}: packed weight is {q.out_features} x {q.in_features}, the "
                             f"model's linear is {lin.out_features} x {lin.in_features}")
        _set_submodule(model, name, q)
        used.update(v for v in keys.values() if v in tensors)
    return _load_rest(model, tensors, used, device)


def _load_rest(model: torch.nn.Module, tensors: Dict[str, torch.Tensor], used, device):
    """Every tensor the packed modules did not take, loaded as is."""
    rest = {k: v for k, v in tensors.items() if k not in used}
    missing, unexpected = model.load_state_dict(rest, strict=False)
    missing = [k for k in missing if k not in used]
    if unexpected:
        raise KeyError(f"checkpoint tensors without a place in the model: {sorted(unexpected)}")
    if missing:
        # tied parameters are saved once per name, so nothing should be missing
        raise KeyError(f"model tensors missing from the checkpoint: {sorted(missing)}")
    if device is not None:
        model.to(device)
    return model
