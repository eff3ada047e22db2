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

Mixture of Experts (A19): an experts module (3-D ``gate_up_proj`` (E, 2I, H) and
``down_proj`` (E, H, I)) is packed as two stacks.  `packed` holds them under the
parameters' names, ``<experts>.gate_up_proj`` and ``<experts>.down_proj``, each
with 3-D ``qweight`` (E, in*b/32, out), ``qzeros`` (E, G, out*b/32) and ``scales``
(E, G, out) (MXFP4: ``qweight`` and uint8 ``scales`` (E, in/32, out)); expert e's
slice is exactly the 2-D image above.  They are written as
``<experts>.gate_up_qweight`` ... ``<experts>.down_scales`` (the buffers of
``qlinear.QuantExperts``; no ``g_idx``) in place of the two parameters, and
``quantize_config.json`` lists the module names under ``"experts"``.  Checkpoints
without the key are read exactly as before.

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
    experts = set()
    for name, t in packed.items():
        if t["qweight"].dim() == 3:              # a stack of an experts module
            mod, _, leaf = name.rpartition(".")
            if leaf not in ("gate_up_proj", "down_proj"):
                raise ValueError(f"{name}: a stacked entry must be named gate_up_proj or down_proj")
            if f"{mod}.gate_up_proj" not in packed or f"{mod}.down_proj" not in packed:
                raise ValueError(f"{mod}: gate_up_proj and down_proj come together")
            if mx and t["scales"].dtype != torch.uint8:
                raise ValueError(f"{name}: MXFP4 scales must be uint8, got {t['scales'].dtype}")
            stem = f"{mod}.{leaf[:-len('_proj')]}"
            tensors[f"{stem}_qweight"] = t["qweight"].contiguous().cpu()
            tensors[f"{stem}_scales"] = (t["scales"] if mx else t["scales"].to(scale_dtype)) \
                .contiguous().cpu()
            if not mx:
                tensors[f"{stem}_qzeros"] = t["qzeros"].contiguous().cpu()
            experts.add(mod)
            continue
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
        if (mod in packed and k.endswith(".weight")) or (mod in experts and k in packed):
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
    if experts:
        qc["experts"] = sorted(experts)
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


def _load_experts(model: torch.nn.Module, tensors: Dict[str, torch.Tensor], qc: Dict[str, Any],
                  used: set, act_format=None) -> None:
    """Every module listed under ``"experts"`` becomes a ``qlinear.QuantExperts``
    holding its two packed stacks, with `act_format` as its activation format;
    `used` gains the tensors taken."""
    from .qlinear import QuantExperts
    mx = qc.get("checkpoint_format") == "mxfp4"
    for name in qc.get("experts", []):
        try:
            mod = model.get_submodule(name)
        except AttributeError:
            raise KeyError(f"{name}: packed in the checkpoint but absent from the model") from None
        if not _is_experts(mod):
            raise TypeError(f"{name}: expected an experts module with 3-D gate_up_proj and "
                            f"down_proj, found {type(mod).__name__}")
        stacks = []
        for stem in ("gate_up", "down"):
            keys = {k: f"{name}.{stem}_{k}" for k in (("qweight", "scales") if mx else
                                                      ("qweight", "qzeros", "scales"))}
            for k in keys.values():
                if k not in tensors:
                    raise KeyError(f"{k} is missing from the checkpoint")
            stacks.append({k: tensors[v] for k, v in keys.items()})
            used.update(keys.values())
        try:
            q = QuantExperts.from_packed(stacks[0], stacks[1], int(qc["bits"]),
                                         int(qc["group_size"]), "mxfp4" if mx else "int",
                                         act_fn=getattr(mod, "act_fn", None),
                                         device=mod.gate_up_proj.device, act_format=act_format)
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
        if (q.num_experts, 2 * q.intermediate_dim, q.hidden_dim) != tuple(mod.gate_up_proj.shape):
            raise ValueError(f"{name}: packed stacks are for gate_up_proj "
                             f"{(q.num_experts, 2 * q.intermediate_dim, q.hidden_dim)}, the "
                             f"model's is {tuple(mod.gate_up_proj.shape)}")
        _set_submodule(model, name, q)


def _is_experts(mod: torch.nn.Module) -> bool:
    """An experts module by duck type: 3-D parameters gate_up_proj and down_proj."""
    gu, dn = getattr(mod, "gate_up_proj", None), getattr(mod, "down_proj", None)
    return isinstance(gu, torch.Tensor) and isinstance(dn, torch.Tensor) \
        and gu.dim() == 3 and dn.dim() == 3


def _set_submodule(model: torch.nn.Module, name: str, new: torch.nn.Module) -> None:
    parent_name, _, leaf = name.rpartition(".")
    parent = model.get_submodule(parent_name) if parent_name else model
    setattr(parent, leaf, new)


def load_quantized(model: torch.nn.Module, path: str, device=None,
                   act_format=None, act_order: bool = False,
                   experts_act_format=None) -> torch.nn.Module:
    """Load a checkpoint written by save_quantized into `model` (the dense
    architecture, any weights) and return it: every ``nn.Linear`` whose
    ``<name>.qweight`` is in the checkpoint becomes a ``qlinear.QuantLinear``
    holding the packed tensors (bias kept, in the linear's dtype); every other
    tensor is loaded as is.  A linear with ``<name>.lr_a`` / ``<name>.lr_b`` gets
    them as its low-rank correction, and one listed in the ``"rotation"`` entry its
    ``had_sign`` and block (the module then rotates its input).  Every module listed
    under ``"experts"`` becomes a ``qlinear.QuantExperts`` with the two packed stacks.
    ``quantize_config.json`` must be a static-group
    ``desc_act=false`` configuration with supported bits, and every ``g_idx``
    must be the trivial ``arange(in) // group`` map (act-order checkpoints are
    out of scope).  `device`: where the model is moved (default: it stays).
    `act_format`: a run-time choice that the checkpoint does not record, handed
    to every packed linear.  None: 16-bit activations.  "mxfp8": the block-scaled
    W4A8 kernel of ``MXQuantLinear``, for MXFP4 checkpoints only.  "int8":
    per-token INT8 activations on the i8 MFMA (``QuantLinear``), for integer
    (``gptq_v2``) checkpoints only.  A format with the other kind of checkpoint,
    an unknown format, and any format with a Mixture-of-Experts checkpoint are a
    ``ValueError`` before any tensor is read.
    ``act_order=True`` lifts the two refusals for integer checkpoints:
    ``desc_act=true`` is accepted, and a linear whose ``g_idx`` is any map with
    `group_size` columns in every group is sorted by group as it is loaded
    (``QuantLinear.from_packed(..., act_order=True)``).  The sort is a kernel, so
    such a layer is built on `device` when that is given and on the model's device
    otherwise, and one of them must be a GPU.  MXFP4 and experts checkpoints have
    no ``g_idx``; nothing changes for them.
    `experts_act_format`: the same run-time choice for the ``QuantExperts`` modules
    alone (the packed linears keep `act_format`).  None: 16-bit activations.
    "mxfp8": both grouped GEMMs of every experts module run on the block-scaled
    MFMA, for MXFP4 checkpoints only; anything else, and "mxfp8" with an integer
    checkpoint, are a ``ValueError`` before any tensor is read."""
    from .qlinear import (ACT_FORMATS, INT_ACT_FORMATS, MXQuantLinear, QuantLinear,
                          _check_act_format)
    if experts_act_format is not None:           # before any tensor is read
        _check_act_format(experts_act_format, ACT_FORMATS, " for experts_act_format")
        with open(os.path.join(path, "quantize_config.json")) as f:
            fmt = json.load(f).get("checkpoint_format", "gptq_v2")
        if fmt != "mxfp4":
            raise ValueError(f"experts_act_format={experts_act_format!r} needs an mxfp4 "
                             f"checkpoint; this one is {fmt!r}")
    if act_format is not None:                   # before any tensor is read
        known = sorted(ACT_FORMATS) + sorted(INT_ACT_FORMATS)
        if not isinstance(act_format, str) or act_format not in known:
            raise ValueError(f"act_format must be None or one of {known}, got {act_format!r}")
        with open(os.path.join(path, "quantize_config.json")) as f:
            head = json.load(f)
        fmt = head.get("checkpoint_format", "gptq_v2")
        if act_format in ACT_FORMATS and fmt != "mxfp4":
            raise ValueError(f"act_format={act_format!r} needs an mxfp4 checkpoint; this one is "
                             f"{fmt!r}")
        if act_format in INT_ACT_FORMATS and fmt != "gptq_v2":
            raise ValueError(f"act_format={act_format!r} needs an integer (gptq_v2) checkpoint; "
                             f"this one is {fmt!r}")
        if head.get("experts"):
            raise ValueError("act_format cannot be combined with a Mixture-of-Experts checkpoint "
                             "(the grouped kernel takes 16-bit activations)")
    tensors, qc = read_quantized(path)
    bits, group = int(qc["bits"]), int(qc["group_size"])
    blocks = _rotation_blocks(qc, tensors)
    if qc.get("checkpoint_format") == "mxfp4":
        if bits != 4 or group != 32:
            raise ValueError(f"quantize_config.json: mxfp4 needs bits=4 and group_size=32, got "
                             f"bits={qc['bits']}, group_size={qc['group_size']}")
        if qc.get("desc_act", False):
            raise ValueError("quantize_config.json: desc_act=true (act-order) checkpoints are not "
                             "supported")
        required = ("scales",)

        def build(t, keys, bias, lowrank, rotation, dev):
            return MXQuantLinear.from_packed(t[keys["qweight"]], t[keys["scales"]], bias=bias,
                                             device=dev, act_format=act_format, lowrank=lowrank,
                                             rotation=rotation)
    else:
        if bits not in (2, 3, 4, 8):
            raise ValueError(f"quantize_config.json: bits={bits} is not one of 2, 3, 4, 8")
        if qc.get("desc_act", False) and not act_order:
            raise ValueError("quantize_config.json: desc_act=true (act-order) checkpoints are not "
                             "supported")
        if not isinstance(qc.get("sym"), bool):
            raise ValueError("quantize_config.json: sym must be true or false")
        fmt = qc.get("checkpoint_format", "gptq_v2")
        if fmt != "gptq_v2":
            raise ValueError(f"quantize_config.json: checkpoint_format={fmt!r}; only gptq_v2 "
                             "(true zero points) and mxfp4 are supported")
        required = ("qzeros", "scales", "g_idx")

        def build(t, keys, bias, lowrank, rotation, dev):
            if act_order and device is not None:
                dev = device               # an act-order layer is sorted where it will run
            return QuantLinear.from_packed(t[keys["qweight"]], t[keys["qzeros"]], t[keys["scales"]],
                                           bits, group, bias=bias, g_idx=t[keys["g_idx"]],
                                           device=dev, lowrank=lowrank, rotation=rotation,
                                           act_format=act_format, act_order=act_order)
    used = set()
    _load_experts(model, tensors, qc, used, experts_act_format)
    _load_linears(model, tensors, used, blocks, required, build)
    return _load_rest(model, tensors, used, device)


def _load_linears(model: torch.nn.Module, tensors: Dict[str, torch.Tensor], used: set,
                  blocks: Dict[str, int], required, build) -> None:
    """Every ``nn.Linear`` with a ``<name>.qweight`` in the checkpoint becomes
    the packed module that ``build(tensors, keys, bias, lowrank, rotation,
    device)`` makes of it (the format's one ``from_packed`` call); `required`
    names the tensors besides ``qweight`` that the format cannot do without, and
    `used` gains the tensors taken."""
    for name in [k[:-len(".qweight")] for k in tensors if k.endswith(".qweight")]:
        try:
            lin = model.get_submodule(name)
        except AttributeError:
            raise KeyError(f"{name}: packed in the checkpoint but absent from the model") from None
        if not isinstance(lin, torch.nn.Linear):
            raise TypeError(f"{name}: expected nn.Linear, found {type(lin).__name__}")
        keys = {k: f"{name}.{k}" for k in ("qweight", *required, "bias")}
        for k in required:
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
            q = build(tensors, keys, bias, lowrank, rotation, lin.weight.device)
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
        if (q.out_features, q.in_features) != (lin.out_features, lin.in_features):
            raise ValueError(f"{name}: packed weight is {q.out_features} x {q.in_features}, the "
                             f"model's linear is {lin.out_features} x {lin.in_features}")
        _set_submodule(model, name, q)
        used.update(v for v in keys.values() if v in tensors)


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
