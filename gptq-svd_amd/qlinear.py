"""Packed-weight inference (A14): the consumer of the checkpoint that
``export.save_quantized`` writes.

``dequantize_packed`` decodes the AutoGPTQ ``gptq_v2`` tensors back into the
dense weight (``tg_dequant_packed``); ``QuantLinear`` keeps them packed and
runs ``y = x W^T + bias`` straight from the packed words (``tg_qgemm``: a
split-K GEMV for up to 16 rows, an MFMA tile kernel above).  Both are HIP
kernels; there is no CPU or eager fallback.

Layout (export.py): ``qweight`` int32 (in*b/32, out), ``qzeros`` int32
(G, out*b/32), ``scales`` fp16 or fp32 (G, out), ``g_idx`` int32 (in,) -- by
default only the trivial map ``arange(in) // group`` (static groups, original
column order).  w = (code_u - zero_u) * scale.

Act-order checkpoints (A21, opt-in with ``act_order=True``): ``g_idx[c]`` is the
group of column c, any map that gives every group exactly ``group`` columns.
The packed stream is sorted by group once at load (``tg_repack_gidx``) and the
forward permutes the activation columns instead (``tg_qgemm_gidx``: fused into
the GEMV's staging at decode, one ``tg_gather_cols`` launch in front of the
tile kernel above), so the hot loops still fetch one zero and one scale per
unit of 32 values; ``tg_dequant_gidx`` returns the original column order.

MXFP4 checkpoints (``checkpoint_format: "mxfp4"``) hold ``qweight`` int32
(in/8, out), the same 4-bit stream of E2M1 codes, and ``scales`` uint8
(in/32, out), the E8M0 byte of each group of 32 input columns; no ``qzeros``
and no ``g_idx``.  w = +-{0, .5, 1, 1.5, 2, 3, 4, 6}[code & 7] * 2^(byte - 127).
``dequantize_packed_mx`` and ``MXQuantLinear`` are their consumers
(``tg_dequant_mx``, ``tg_qgemm_mx``).

MXFP8 activations (A16, opt-in): ``MXQuantLinear(..., act_format="mxfp8")``
quantises x to e4m3 with one E8M0 byte per 32 columns (``quantize_act_mx``,
``tg_quant_act_mx``) and multiplies on the block-scaled MFMA instruction
(``tg_qgemm_mx_act``): W4A8, different numerics from the weights-only path.

INT8 activations (A20, opt-in): ``QuantLinear(..., act_format="int8")`` quantises
x per token to int8 (``quantize_act_i8``, ``tg_quant_act_i8``) and multiplies the
packed integer codes on the i8 MFMA (``tg_qgemm_act``): W4A8 (or W2/3/8A8), with
the zero points applied once per group; different numerics from the weights-only
path, and a run-time choice that the checkpoint does not record.

Low-rank correction (A17, opt-in): a layer quantised with ``lowrank=r`` carries
``lr_a`` (out, r) and ``lr_b`` (r, in) beside its packed weight, and computes
``y = x W^^T + (x lr_b^T) lr_a^T + bias`` in three calls: the packed GEMM with
fp32 output and no bias, ``tg_lr_down`` and ``tg_lr_finish``.  Without the two
buffers the forward is the single call it was.

Hadamard rotation (A18, opt-in): a layer quantised with ``rotate`` stores the
weight of the rotated basis, W' = W Q, and carries ``had_sign`` (int32, in/32
words of sign bits) and ``rotate_block``.  Its forward first computes
``x' = x Q`` in the activation dtype (``hadamard``, one ``tg_hadamard`` launch)
and feeds x' to everything that took x: ``y = x' W'^^T (+ (x' lr_b^T) lr_a^T)
+ bias``.

Mixture of Experts (A19): ``QuantExperts`` replaces a layer's experts module
(3-D ``gate_up_proj`` (E, 2I, H) and ``down_proj`` (E, H, I), the layout of
``Qwen3MoeExperts`` / ``MixtralExperts``) and keeps both stacks packed, in either
weight format.  Its forward sorts the token-expert assignments by expert on the
device and runs two ``tg_qgemm_grouped`` calls (``qgemm_grouped``), with no host
synchronisation and no atomics.

Structure: ``QuantLinear`` and ``MXQuantLinear`` derive from ``_PackedLinear``,
which owns the bias / correction / rotation buffers, ``dequantize`` and the
forward around the packed GEMM; a subclass adds its weight buffers, its shape
checks, the decoded weight (``_dense``) and its ``tg_qgemm*`` call (``_gemm``).
``_rows`` is the one place that turns an input into rows with a stride.
``QuantExperts`` stands alone.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from ._lib import (ACT_FORMATS, DTYPES, INT_ACT_FORMATS, TG_FMT_MXFP4, call, lib, ptr,
                   require_cuda, stream, workspace)

__all__ = ["QuantLinear", "dequantize_packed", "MXQuantLinear", "dequantize_packed_mx",
           "quantize_act_mx", "dequantize_act_mx", "add_lowrank", "hadamard", "QuantExperts",
           "qgemm_grouped", "INT_ACT_FORMATS", "quantize_act_i8", "dequantize_act_i8"]

_BITS = (2, 3, 4, 8)


def _rows(x: torch.Tensor, n: int):
    """``(x2, T, ldx)``: x as T rows of width n with unit column stride, a view
    wherever the kernels' row stride ``ldx >= n`` can describe it and a copy
    otherwise."""
    x2 = x.reshape(-1, n)
    T = x2.shape[0]
    if T > 0 and (x2.stride(1) != 1 or (T > 1 and x2.stride(0) < n)):
        x2 = x2.contiguous()
    return x2, T, x2.stride(0) if T > 1 else n


def _shapes(qweight: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor, w_bits: int,
            group_size: int):
    """(m, n, g) of a packed triple, checked against each other."""
    if w_bits not in _BITS:
        raise ValueError(f"w_bits must be one of {_BITS}, got {w_bits}")
    if qweight.dtype != torch.int32 or qzeros.dtype != torch.int32:
        raise ValueError("qweight and qzeros must be int32")
    if scales.dtype not in (torch.float16, torch.float32):
        raise ValueError("scales must be float16 or float32")
    nw, m = qweight.shape
    if (nw * 32) % w_bits:
        raise ValueError(f"qweight has {nw} word rows, not a whole number of {w_bits}-bit values")
    n = nw * 32 // w_bits
    g = group_size if group_size > 0 else n
    if n % g:
        raise ValueError(f"group_size {group_size} does not divide in_features {n}")
    G = n // g
    if tuple(scales.shape) != (G, m) or tuple(qzeros.shape) != (G, m * w_bits // 32):
        raise ValueError(f"packed shapes disagree: qweight {tuple(qweight.shape)}, qzeros "
                         f"{tuple(qzeros.shape)}, scales {tuple(scales.shape)} for bits={w_bits}, "
                         f"group={group_size}")
    return m, n, g


def _gidx_plan(g_idx: torch.Tensor, n: int, g: int) -> Optional[torch.Tensor]:
    """The load-time plan of an act-order layer: ``col_perm = argsort(g_idx,
    stable)`` as a CPU int32 tensor (the columns of group 0 in ascending order,
    then group 1, ...), or None for the trivial map, which is the static layer.
    Every value of `g_idx` must lie in [0, n/g) and every group have g columns."""
    if tuple(g_idx.shape) != (n,):
        raise ValueError(f"g_idx must have shape ({n},), got {tuple(g_idx.shape)}")
    gi = g_idx.detach().cpu().to(torch.int64)
    if torch.equal(gi, torch.arange(n, dtype=torch.int64) // g):
        return None
    G = n // g
    if int(gi.min()) < 0 or int(gi.max()) >= G:
        raise ValueError(f"g_idx has values outside [0, {G}) (in_features {n}, group {g})")
    if not bool((torch.bincount(gi, minlength=G) == g).all()):
        raise ValueError(f"g_idx does not give every group exactly {g} columns")
    return torch.argsort(gi, stable=True).to(torch.int32)


def _repack_gidx(qweight: torch.Tensor, col_perm: torch.Tensor, w_bits: int) -> torch.Tensor:
    """The stream sorted by group: position j holds the code of column
    ``col_perm[j]`` (``tg_repack_gidx``); both tensors on one GPU."""
    require_cuda(qweight, "act-order qweight")
    qweight = qweight.contiguous()
    nw, m = qweight.shape
    out = torch.empty_like(qweight)
    with torch.cuda.device(qweight.device):
        call("tg_repack_gidx", stream(), ptr(qweight), ptr(col_perm), m, nw * 32 // w_bits, w_bits,
             ptr(out))
    return out


def _dequant_gidx(qsorted: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor,
                  col_perm: torch.Tensor, m: int, n: int, g: int, w_bits: int,
                  dtype: torch.dtype) -> torch.Tensor:
    out = torch.empty((m, n), dtype=dtype, device=qsorted.device)
    with torch.cuda.device(qsorted.device):
        call("tg_dequant_gidx", stream(), ptr(qsorted), ptr(qzeros), ptr(scales),
             DTYPES[scales.dtype], m, n, g, w_bits, ptr(out), DTYPES[dtype], n, ptr(col_perm))
    return out


def dequantize_packed(qweight: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor,
                      w_bits: int, group_size: int, dtype: torch.dtype = torch.float16,
                      g_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dense weight (out, in) of `dtype` (fp16 / bf16 / fp32):
    ``float(code_u - zero_u) * float(scale)`` rounded once to `dtype`.  With a
    `g_idx` (the tensors in checkpoint layout) column c takes the zero and scale
    of group ``g_idx[c]``: the stream is sorted by group (``tg_repack_gidx``) and
    decoded back into the original column order (``tg_dequant_gidx``)."""
    m, n, g = _shapes(qweight, qzeros, scales, w_bits, group_size)
    col_perm = None if g_idx is None else _gidx_plan(g_idx, n, g)
    if col_perm is not None and n % 32:
        raise ValueError(f"a non-trivial g_idx needs in_features % 32 == 0, got {n}")
    for t, what in ((qweight, "qweight"), (qzeros, "qzeros"), (scales, "scales")):
        require_cuda(t, what)
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"dtype must be float16, bfloat16 or float32, got {dtype}")
    dev = qweight.device
    qweight, qzeros, scales = qweight.contiguous(), qzeros.contiguous(), scales.contiguous()
    if col_perm is not None:
        col_perm = col_perm.to(dev)
        return _dequant_gidx(_repack_gidx(qweight, col_perm, w_bits), qzeros, scales, col_perm,
                             m, n, g, w_bits, dtype)
    out = torch.empty((m, n), dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        call("tg_dequant_packed", stream(), ptr(qweight), ptr(qzeros), ptr(scales),
             DTYPES[scales.dtype], m, n, g, w_bits, ptr(out), DTYPES[dtype], n)
    return out


# ---------------------------------------------------------------------------
# Hadamard rotation (A18)
# ---------------------------------------------------------------------------
_HAD_DTYPES = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def _check_block(block: int, n: int) -> int:
    block = int(block)
    if block < 32 or block > 4096 or block & (block - 1):
        raise ValueError(f"Hadamard block must be a power of two in [32, 4096], got {block}")
    if n % block:
        raise ValueError(f"Hadamard block {block} does not divide the width {n}")
    return block


def hadamard(x: torch.Tensor, block: int, sign_bits: Optional[torch.Tensor],
             inverse: bool = False, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``x Q`` (``x Q^T`` with `inverse`) on the last dim, Q the randomised block
    Hadamard matrix of `block` and `sign_bits` (int32, n/32 words, bit j of word i
    = column 32 i + j is negated; None = all +): one ``tg_hadamard`` launch.
    fp16 / bf16 / fp32 inputs compute in fp32 and round once to `dtype` (default:
    the input's; one of those three); float64 stays float64."""
    require_cuda(x, "hadamard input")
    if x.dtype not in _HAD_DTYPES:
        raise RuntimeError(f"hadamard takes float16, bfloat16, float32 or float64, got {x.dtype}")
    dtype = x.dtype if dtype is None else dtype
    if dtype not in _HAD_DTYPES or (dtype == torch.float64) != (x.dtype == torch.float64):
        raise ValueError(f"hadamard: output dtype {dtype} does not go with input dtype {x.dtype}")
    n = x.shape[-1]
    block = _check_block(block, n)
    if sign_bits is not None:
        require_cuda(sign_bits, "hadamard sign_bits")
        if sign_bits.dtype != torch.int32 or tuple(sign_bits.shape) != (n // 32,):
            raise ValueError(f"sign_bits must be int32 of {n // 32} words, got {sign_bits.dtype} "
                             f"{tuple(sign_bits.shape)}")
        sign_bits = sign_bits.contiguous()
    x2, T, ldx = _rows(x, n)
    y = torch.empty((T, n), dtype=dtype, device=x.device)
    if T > 0:
        with torch.cuda.device(x.device):
            call("tg_hadamard", stream(), ptr(x2), DTYPES[x.dtype], T, n, ldx, block,
                 ptr(sign_bits), int(bool(inverse)), ptr(y), DTYPES[dtype], n)
    return y.reshape(x.shape)


def _rotate_rows(x2: torch.Tensor, T: int, n: int, ldx: int, block: int,
                 sign_bits: torch.Tensor) -> torch.Tensor:
    """x2 Q in x2's dtype, (T, n) contiguous: the one launch a rotated forward adds."""
    xr = torch.empty((T, n), dtype=x2.dtype, device=x2.device)
    with torch.cuda.device(x2.device):
        call("tg_hadamard", stream(), ptr(x2), DTYPES[x2.dtype], T, n, ldx, block, ptr(sign_bits),
             0, ptr(xr), DTYPES[x2.dtype], n)
    return xr


def _check_rotation(rotation, n: int):
    """(block, sign_bits) of a ``rotation=`` argument, checked against the width."""
    block, sign = rotation
    block = _check_block(block, n)
    if sign.dtype != torch.int32 or tuple(sign.shape) != (n // 32,):
        raise ValueError(f"rotation sign_bits must be int32 of {n // 32} words, got {sign.dtype} "
                         f"{tuple(sign.shape)}")
    return block, sign


# ---------------------------------------------------------------------------
# Low-rank correction (A17)
# ---------------------------------------------------------------------------
_LR_DTYPES = (torch.float16, torch.bfloat16, torch.float32)


def _check_lowrank(lowrank, m: int, n: int):
    """(A, B) of a ``lowrank=`` argument, checked against the layer's shape."""
    A, B = lowrank
    if A.dim() != 2 or B.dim() != 2 or A.shape[0] != m or B.shape[1] != n \
            or A.shape[1] != B.shape[0]:
        raise ValueError(f"lowrank factors {tuple(A.shape)}, {tuple(B.shape)} do not fit a "
                         f"({m}, {n}) weight")
    if not 1 <= A.shape[1] <= 128:
        raise ValueError(f"lowrank rank must be in [1, 128], got {A.shape[1]}")
    if A.dtype not in _LR_DTYPES or B.dtype not in _LR_DTYPES:
        raise ValueError("lowrank factors must be float16, bfloat16 or float32")
    return A, B


def _lowrank_finish(x2: torch.Tensor, T: int, ldx: int, y32: torch.Tensor, lr_a: torch.Tensor,
                    lr_b: torch.Tensor, bias: Optional[torch.Tensor], y: torch.Tensor) -> None:
    """y = round(y32 + (x2 lr_b^T) lr_a^T + bias): tg_lr_down, tg_lr_finish.  Call
    inside ``torch.cuda.device``."""
    m, r = lr_a.shape
    n = lr_b.shape[1]
    if lr_a.stride(1) != 1 or lr_b.stride(1) != 1:
        lr_a, lr_b = lr_a.contiguous(), lr_b.contiguous()
    z = torch.empty((T, r), dtype=torch.float32, device=y.device)
    nbytes = lib.tg_lr_down_workspace_size(T, r, n)
    ws = workspace(nbytes, y.device)
    call("tg_lr_down", stream(), ptr(x2), DTYPES[x2.dtype], T, ldx, ptr(lr_b), DTYPES[lr_b.dtype],
         r, n, lr_b.stride(0), ptr(z), r, ptr(ws), nbytes)
    call("tg_lr_finish", stream(), ptr(y32), y32.stride(0), ptr(z), r, ptr(lr_a),
         DTYPES[lr_a.dtype], lr_a.stride(0), T, m, r, ptr(bias),
         DTYPES[bias.dtype] if bias is not None else 0, ptr(y), DTYPES[y.dtype], y.stride(0))


def add_lowrank(W: torch.Tensor, A: torch.Tensor, B: torch.Tensor,
                dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``W + A B`` as the packed forward applies it, as a dense (out, in) matrix:
    each entry starts from float32 W[o, i] and adds A[o, j] B[j, i] in ascending j
    as fp32 fmas, then rounds once to `dtype` (``tg_lr_finish`` with the output
    features as its rows).  The harness writes this back for a layer quantised
    with ``lowrank``, and ``dequantize(effective=True)`` returns it."""
    require_cuda(W, "add_lowrank W")
    m, n = W.shape
    A, B = _check_lowrank((A, B), m, n)
    if dtype not in _LR_DTYPES:
        raise ValueError(f"dtype must be float16, bfloat16 or float32, got {dtype}")
    dev = W.device
    W32 = W.to(torch.float32).contiguous()
    z = A.to(device=dev, dtype=torch.float32).contiguous()        # exact
    Bt = B.to(device=dev).t().contiguous()                         # (in, r)
    r = z.shape[1]
    out = torch.empty((m, n), dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        call("tg_lr_finish", stream(), ptr(W32), n, ptr(z), r, ptr(Bt), DTYPES[Bt.dtype], r, m, n,
             r, None, 0, ptr(out), DTYPES[dtype], n)
    return out


def _check_act_format(act_format, allowed, where: str = "") -> None:
    """None or a key of `allowed`; `where` names the kind of checkpoint that
    takes only these."""
    if act_format is not None and (not isinstance(act_format, str) or act_format not in allowed):
        raise ValueError(f"act_format must be None or one of {sorted(allowed)}{where}, got "
                         f"{act_format!r}")


def quantize_act_i8(x: torch.Tensor):
    """Per-token INT8 image of fp16 / bf16 activations (..., n), n % 32 == 0:
    ``(xq int8 (..., n), xs float32 (...))`` with ``xs = max|x| / 127`` and
    ``xq = rint(x / xs)`` in [-127, 127] (``tg_quant_act_i8``)."""
    require_cuda(x, "quantize_act_i8 input")
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError(f"quantize_act_i8 takes float16 or bfloat16, got {x.dtype}")
    n = x.shape[-1]
    if n == 0 or n % 32:
        raise ValueError(f"quantize_act_i8 needs a last dim that is a multiple of 32, got {n}")
    x2, T, ldx = _rows(x, n)
    xq = torch.empty((T, n), dtype=torch.int8, device=x.device)
    xs = torch.empty((T,), dtype=torch.float32, device=x.device)
    if T > 0:
        with torch.cuda.device(x.device):
            call("tg_quant_act_i8", stream(), ptr(x2), DTYPES[x.dtype], T, ldx, n, 32, ptr(xq), n,
                 ptr(xs), None)
    return xq.reshape(*x.shape[:-1], n), xs.reshape(x.shape[:-1])


def dequantize_act_i8(xq: torch.Tensor, xs: torch.Tensor,
                      dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``float(xq) * xs`` rounded once to `dtype` (plain torch)."""
    return (xq.to(torch.float32) * xs.unsqueeze(-1)).to(dtype)


class _PackedLinear(nn.Module):
    """What ``QuantLinear`` and ``MXQuantLinear`` share: the optional buffers
    (bias, low-rank correction, rotation) and everything around the one packed
    GEMM of a forward.  A subclass registers its weight buffers, then calls
    ``_register_extras``, and supplies ``_dense`` (the decoded weight) and
    ``_gemm`` (its ``tg_qgemm*`` call)."""

    def _register_extras(self, bias: bool, bias_dtype: torch.dtype, lowrank: int,
                         lowrank_dtype: torch.dtype, rotate_block: int, device) -> None:
        """Buffers ``bias`` (out,), ``lr_a`` (out, r) and ``lr_b`` (r, in), and
        ``had_sign`` (int32, in/32 words) with ``rotate_block``; whatever is absent
        is a None attribute."""
        n, m = self.in_features, self.out_features
        if bias:
            self.register_buffer("bias", torch.zeros(m, dtype=bias_dtype, device=device))
        else:
            self.bias = None
        if lowrank:
            if not 1 <= lowrank <= 128:
                raise ValueError(f"lowrank must be in [0, 128], got {lowrank}")
            if lowrank_dtype not in _LR_DTYPES:
                raise ValueError("lowrank_dtype must be float16, bfloat16 or float32")
            self.register_buffer("lr_a", torch.zeros((m, lowrank), dtype=lowrank_dtype,
                                                     device=device))
            self.register_buffer("lr_b", torch.zeros((lowrank, n), dtype=lowrank_dtype,
                                                     device=device))
        else:
            self.lr_a = self.lr_b = None
        self.rotate_block = int(rotate_block)
        if self.rotate_block:
            _check_block(rotate_block, n)
            self.register_buffer("had_sign", torch.zeros(n // 32, dtype=torch.int32, device=device))
        else:
            self.had_sign = None

    @staticmethod
    def _extras_args(m: int, n: int, bias, lowrank, rotation) -> dict:
        """The constructor's keywords for the ``bias=``, ``lowrank=`` and
        ``rotation=`` of a ``from_packed``, the last two checked against (m, n)."""
        kw = dict(lowrank=0, lowrank_dtype=torch.float16, rotate_block=0)
        if lowrank is not None:
            A, _ = _check_lowrank(lowrank, m, n)
            kw.update(lowrank=A.shape[1], lowrank_dtype=A.dtype)
        if rotation is not None:
            kw.update(rotate_block=_check_rotation(rotation, n)[0])
        return dict(kw, bias=bias is not None,
                    bias_dtype=bias.dtype if bias is not None else torch.float16)

    def _fill(self, weights: dict, bias, lowrank, rotation):
        """Copy a ``from_packed``'s tensors into the buffers; returns self."""
        for name, t in weights.items():
            getattr(self, name).copy_(t)
        if bias is not None:
            self.bias.copy_(bias.detach())
        if lowrank is not None:
            self.lr_a.copy_(lowrank[0].detach())
            self.lr_b.copy_(lowrank[1].detach())
        if rotation is not None:
            self.had_sign.copy_(rotation[1])
        return self

    def _extras_repr(self) -> str:
        lr = f", lowrank={self.lr_a.shape[1]}" if self.lr_a is not None else ""
        return lr + (f", rotate_block={self.rotate_block}" if self.rotate_block else "")

    def dequantize(self, dtype: torch.dtype = torch.float16, effective: bool = False,
                   rotated: bool = True) -> torch.Tensor:
        """The dense (out, in) weight; ``effective=True`` adds the low-rank
        correction, W^ + lr_a lr_b (``add_lowrank``), when the layer has one.
        A rotated layer stores the weight of the rotated basis, and that is what
        ``rotated=True`` returns; ``rotated=False`` returns R^-1 of it (computed
        from the fp32 matrix, rounded once to `dtype`), the matrix for which
        ``x @ W.T`` approximates the forward."""
        back = self.rotate_block and not rotated
        dt = torch.float32 if back else dtype
        if effective and self.lr_a is not None:
            W = add_lowrank(self._dense(torch.float32), self.lr_a, self.lr_b, dt)
        else:
            W = self._dense(dt)
        return hadamard(W, self.rotate_block, self.had_sign, inverse=True, dtype=dtype) \
            if back else W

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not (x.is_cuda and self.qweight.is_cuda):    # the names are built off the hot path
            require_cuda(x, f"{type(self).__name__} input")
            require_cuda(self.qweight, f"{type(self).__name__}.qweight")
        if x.dtype not in (torch.float16, torch.bfloat16):
            raise RuntimeError(f"{type(self).__name__} takes float16 or bfloat16 activations, got "
                               f"{x.dtype} (there is no fp32 kernel and no fallback)")
        if x.shape[-1] != self.in_features:
            raise RuntimeError(f"{type(self).__name__}: last dim {x.shape[-1]} != in_features "
                               f"{self.in_features}")
        n, m = self.in_features, self.out_features
        x2, T, ldx = _rows(x, n)
        y = torch.empty((T, m), dtype=x.dtype, device=x.device)
        if T > 0:
            if self.rotate_block:
                x2, ldx = _rotate_rows(x2, T, n, ldx, self.rotate_block, self.had_sign), n
            lr = self.lr_a is not None
            # with a correction the GEMM leaves its fp32 sums; tg_lr_finish adds the bias.
            # Z = x lr_b^T always comes from the 16-bit x, under act_format too.
            out = torch.empty((T, m), dtype=torch.float32, device=x.device) if lr else y
            with torch.cuda.device(x.device):
                self._gemm(x2, T, ldx, None if lr else self.bias, out)
                if lr:
                    _lowrank_finish(x2, T, ldx, out, self.lr_a, self.lr_b, self.bias, y)
        return y.reshape(*x.shape[:-1], m)


class QuantLinear(_PackedLinear):
    """A linear layer whose weight stays packed.  The buffer names are the
    checkpoint's keys, so ``load_state_dict`` fills it.  ``module.to(dtype)``
    converts floating buffers like any module: fp32 ``scales`` become 16-bit
    with it (and the decoded weight changes accordingly).
    ``act_format=None``: weights only, the codes are decoded to x's dtype
    (``tg_qgemm``).  ``act_format="int8"``: x is quantised per token to int8 per
    call and both operands feed the i8 MFMA (``tg_qgemm_act``); a run-time choice
    that the checkpoint does not record.
    An act-order layer (``from_packed(..., act_order=True)`` with a non-trivial
    `g_idx`) holds the stream sorted by group in ``qweight``, the checkpoint's
    map in ``g_idx`` and ``col_perm = argsort(g_idx)`` as a non-persistent
    buffer (None for a static layer).  Its ``state_dict()`` therefore holds the
    sorted stream beside the unsorted map: it is not a checkpoint, and loading it
    anywhere, into another ``QuantLinear`` included, decodes the wrong weight."""

    def __init__(self, in_features: int, out_features: int, w_bits: int, group_size: int,
                 bias: bool = False, scale_dtype: torch.dtype = torch.float16,
                 bias_dtype: torch.dtype = torch.float16, device=None, lowrank: int = 0,
                 lowrank_dtype: torch.dtype = torch.float16, rotate_block: int = 0,
                 act_format=None):
        super().__init__()
        _check_act_format(act_format, INT_ACT_FORMATS, " for an integer checkpoint")
        self.act_format = act_format
        if w_bits not in _BITS:
            raise ValueError(f"w_bits must be one of {_BITS}, got {w_bits}")
        g = group_size if group_size > 0 else in_features
        if in_features % 32 or g % 32 or in_features % g or (out_features * w_bits) % 32:
            raise ValueError(
                f"QuantLinear needs in_features % 32 == 0, group % 32 == 0 dividing in_features "
                f"and out_features * bits % 32 == 0 (got in={in_features}, out={out_features}, "
                f"group={group_size}, bits={w_bits})")
        self.in_features, self.out_features = int(in_features), int(out_features)
        self.w_bits, self.group_size = int(w_bits), int(group_size)
        G = in_features // g
        self.register_buffer("qweight", torch.zeros((in_features * w_bits // 32, out_features),
                                                    dtype=torch.int32, device=device))
        self.register_buffer("qzeros", torch.zeros((G, out_features * w_bits // 32),
                                                   dtype=torch.int32, device=device))
        self.register_buffer("scales", torch.zeros((G, out_features), dtype=scale_dtype,
                                                   device=device))
        self.register_buffer("g_idx", (torch.arange(in_features, dtype=torch.int32,
                                                    device=device) // g).to(torch.int32))
        self.register_buffer("col_perm", None, persistent=False)
        self._register_extras(bias, bias_dtype, int(lowrank), lowrank_dtype, rotate_block, device)

    @classmethod
    def from_packed(cls, qweight: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor,
                    w_bits: int, group_size: int, bias: Optional[torch.Tensor] = None,
                    g_idx: Optional[torch.Tensor] = None, device=None,
                    lowrank=None, rotation=None, act_format=None,
                    act_order: bool = False) -> "QuantLinear":
        """From the packed tensors (a checkpoint's, or ``pack_quantized``'s).
        `g_idx`, when given, must be the trivial ``arange(in) // group``, unless
        ``act_order=True``: then any map with `group_size` columns in every group
        is taken, `qweight` is sorted by group once, on the module's device (a
        GPU), and the forward gathers x through ``col_perm``; a trivial map still
        gives the static module.  ``act_format`` does not go with such a map.
        ``lowrank=(A, B)``: the correction's factors, (out, r) and (r, in).
        ``rotation=(block, sign_bits)``: the packed weight is that of the rotated
        basis and the forward rotates x first.  ``act_format``: None or "int8"."""
        m, n, g = _shapes(qweight, qzeros, scales, w_bits, group_size)
        extras = cls._extras_args(m, n, bias, lowrank, rotation)
        col_perm = None
        if g_idx is not None and act_order:
            col_perm = _gidx_plan(g_idx, n, g)
            if col_perm is not None and act_format is not None:
                raise ValueError(f"act_format={act_format!r} cannot be combined with an act-order "
                                 "g_idx (the INT8 kernel sums groups of consecutive columns)")
        elif g_idx is not None:
            triv = torch.arange(n, dtype=torch.int64) // g
            if tuple(g_idx.shape) != (n,) or not torch.equal(g_idx.cpu().to(torch.int64), triv):
                raise ValueError("g_idx is not the static arange(in_features) // group_size map "
                                 "(act-order checkpoints are not supported)")
        dev = device if device is not None else qweight.device
        q = cls(n, m, w_bits, group_size, scale_dtype=scales.dtype, device=dev,
                act_format=act_format, **extras)
        if col_perm is not None:
            q.col_perm = col_perm.to(dev)
            qweight = _repack_gidx(qweight.to(dev), q.col_perm, w_bits)
            q.g_idx.copy_(g_idx)
        return q._fill(dict(qweight=qweight, qzeros=qzeros, scales=scales), bias, lowrank, rotation)

    def extra_repr(self) -> str:
        act = f", act_format={self.act_format}" if self.act_format is not None else ""
        act += ", act_order=True" if self.col_perm is not None else ""
        return (f"in_features={self.in_features}, out_features={self.out_features}, "
                f"bits={self.w_bits}, group_size={self.group_size}, "
                f"bias={self.bias is not None}{self._extras_repr()}{act}")

    def _dense(self, dtype: torch.dtype) -> torch.Tensor:
        if self.col_perm is not None:
            if dtype not in (torch.float16, torch.bfloat16, torch.float32):
                raise ValueError(f"dtype must be float16, bfloat16 or float32, got {dtype}")
            require_cuda(self.qweight, "QuantLinear.qweight")
            n, m = self.in_features, self.out_features
            return _dequant_gidx(self.qweight, self.qzeros, self.scales, self.col_perm, m, n,
                                 self.group_size if self.group_size > 0 else n, self.w_bits, dtype)
        return dequantize_packed(self.qweight, self.qzeros, self.scales, self.w_bits,
                                 self.group_size, dtype)

    def _gemm(self, x2: torch.Tensor, T: int, ldx: int, bias: Optional[torch.Tensor],
              out: torch.Tensor) -> None:
        n, m = self.in_features, self.out_features
        if self.col_perm is not None:
            nbytes = lib.tg_qgemm_gidx_workspace_size(T, m, n)
            ws = workspace(nbytes, x2.device)
            call("tg_qgemm_gidx", stream(), ptr(x2), DTYPES[x2.dtype], T, ldx,
                 ptr(self.qweight), ptr(self.qzeros), ptr(self.scales),
                 DTYPES[self.scales.dtype], m, n, self.group_size, self.w_bits, ptr(bias),
                 DTYPES[bias.dtype] if bias is not None else 0, ptr(out), DTYPES[out.dtype], m,
                 ptr(ws), nbytes, ptr(self.col_perm))
        elif self.act_format is not None:
            nbytes = lib.tg_qgemm_act_workspace_size(T, m, n, self.group_size)
            ws = workspace(nbytes, x2.device)
            call("tg_qgemm_act", stream(), ptr(x2), DTYPES[x2.dtype], T, ldx,
                 ptr(self.qweight), ptr(self.qzeros), ptr(self.scales),
                 DTYPES[self.scales.dtype], m, n, self.group_size, self.w_bits,
                 INT_ACT_FORMATS[self.act_format], ptr(bias),
                 DTYPES[bias.dtype] if bias is not None else 0, ptr(out), DTYPES[out.dtype], m,
                 ptr(ws), nbytes)
        else:
            nbytes = lib.tg_qgemm_workspace_size(T, m, n)
            ws = workspace(nbytes, x2.device)
            call("tg_qgemm", stream(), ptr(x2), DTYPES[x2.dtype], T, ldx,
                 ptr(self.qweight), ptr(self.qzeros), ptr(self.scales),
                 DTYPES[self.scales.dtype], m, n, self.group_size, self.w_bits, ptr(bias),
                 DTYPES[bias.dtype] if bias is not None else 0, ptr(out), DTYPES[out.dtype], m,
                 ptr(ws), nbytes)


# ---------------------------------------------------------------------------
# MXFP4 (A15)
# ---------------------------------------------------------------------------
def _shapes_mx(qweight: torch.Tensor, scales: torch.Tensor):
    """(m, n) of an MXFP4 pair, checked against each other."""
    if qweight.dtype != torch.int32:
        raise ValueError("qweight must be int32")
    if scales.dtype != torch.uint8:
        raise ValueError(f"MXFP4 scales must be uint8 (E8M0 bytes), got {scales.dtype}")
    if qweight.dim() != 2 or scales.dim() != 2:
        raise ValueError("qweight and scales must be matrices")
    nw, m = qweight.shape
    n = nw * 8
    if n % 32 or (m * 4) % 32:
        raise ValueError(f"MXFP4 needs in_features % 32 == 0 and out_features % 8 == 0 (got "
                         f"in={n}, out={m})")
    if tuple(scales.shape) != (n // 32, m):
        raise ValueError(f"packed shapes disagree: qweight {tuple(qweight.shape)}, scales "
                         f"{tuple(scales.shape)} (expected {(n // 32, m)})")
    return m, n


def dequantize_packed_mx(qweight: torch.Tensor, scales: torch.Tensor,
                         dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """Dense weight (out, in) of `dtype` (fp16 / bf16 / fp32) of an MXFP4 pair:
    ``grid[code] * 2^(byte - 127)`` rounded once to `dtype`.  fp16 overflows to
    inf for scale bytes from 141 up; bf16 and fp32 cover every byte."""
    m, n = _shapes_mx(qweight, scales)
    for t, what in ((qweight, "qweight"), (scales, "scales")):
        require_cuda(t, what)
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"dtype must be float16, bfloat16 or float32, got {dtype}")
    dev = qweight.device
    qweight, scales = qweight.contiguous(), scales.contiguous()
    out = torch.empty((m, n), dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        call("tg_dequant_mx", stream(), ptr(qweight), ptr(scales), TG_FMT_MXFP4, m, n, ptr(out),
             DTYPES[dtype], n)
    return out


def quantize_act_mx(x: torch.Tensor):
    """MXFP8 image of fp16 / bf16 activations (..., n), n % 32 == 0:
    ``(xq uint8 (..., n), xs uint8 (..., n/32))``, e4m3fn bytes (OCP) and the
    E8M0 byte of each block of 32 columns (``tg_quant_act_mx``)."""
    require_cuda(x, "quantize_act_mx input")
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError(f"quantize_act_mx takes float16 or bfloat16, got {x.dtype}")
    n = x.shape[-1]
    if n == 0 or n % 32:
        raise ValueError(f"quantize_act_mx needs a last dim that is a multiple of 32, got {n}")
    x2, T, ldx = _rows(x, n)
    xq = torch.empty((T, n), dtype=torch.uint8, device=x.device)
    xs = torch.empty((T, n // 32), dtype=torch.uint8, device=x.device)
    if T > 0:
        with torch.cuda.device(x.device):
            call("tg_quant_act_mx", stream(), ptr(x2), DTYPES[x.dtype], T, ldx, n,
                 ACT_FORMATS["mxfp8"], ptr(xq), n, ptr(xs))
    return xq.reshape(*x.shape[:-1], n), xs.reshape(*x.shape[:-1], n // 32)


def dequantize_act_mx(xq: torch.Tensor, xs: torch.Tensor,
                      dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``float(e4m3(xq)) * 2^(xs - 127)`` rounded once to `dtype` (plain torch;
    exact in fp32, and in bf16 for every block scale bf16 can hold)."""
    v = xq.view(torch.float8_e4m3fn).to(torch.float32)
    e = xs.to(torch.int32)
    # 2^(byte - 127) built in the exponent field; byte 0 is the subnormal 2^-127
    s = torch.where(e > 0, e << 23, torch.full_like(e, 0x00400000)).view(torch.float32)
    return (v * s.repeat_interleave(32, dim=-1)).to(dtype)


class MXQuantLinear(_PackedLinear):
    """A linear layer whose weight stays packed as MXFP4: buffers ``qweight``
    int32 (in/8, out) and ``scales`` uint8 (in/32, out), the checkpoint's keys.
    ``act_format=None``: weights only, activations are fp16 / bf16 and the
    decoded weight feeds the 16-bit kernels of ``QuantLinear`` (``tg_qgemm_mx``).
    ``act_format="mxfp8"``: the activations are quantised to MXFP8 per call and
    both operands feed the block-scaled MFMA (``tg_qgemm_mx_act``); a run-time
    choice that the checkpoint does not record."""

    w_bits, group_size = 4, 32

    def __init__(self, in_features: int, out_features: int, bias: bool = False,
                 bias_dtype: torch.dtype = torch.float16, device=None, act_format=None,
                 lowrank: int = 0, lowrank_dtype: torch.dtype = torch.float16,
                 rotate_block: int = 0):
        super().__init__()
        _check_act_format(act_format, ACT_FORMATS)
        self.act_format = act_format
        if in_features % 32 or (out_features * 4) % 32:
            raise ValueError(f"MXQuantLinear needs in_features % 32 == 0 and out_features % 8 == 0 "
                             f"(got in={in_features}, out={out_features})")
        self.in_features, self.out_features = int(in_features), int(out_features)
        self.register_buffer("qweight", torch.zeros((in_features // 8, out_features),
                                                    dtype=torch.int32, device=device))
        # byte 127 = scale 1
        self.register_buffer("scales", torch.full((in_features // 32, out_features), 127,
                                                  dtype=torch.uint8, device=device))
        self._register_extras(bias, bias_dtype, int(lowrank), lowrank_dtype, rotate_block, device)

    @classmethod
    def from_packed(cls, qweight: torch.Tensor, scales: torch.Tensor,
                    bias: Optional[torch.Tensor] = None, device=None,
                    act_format=None, lowrank=None, rotation=None) -> "MXQuantLinear":
        """From the packed pair (a checkpoint's, or ``pack_quantized``'s).
        ``lowrank=(A, B)``: the correction's factors, (out, r) and (r, in).
        ``rotation=(block, sign_bits)``: the packed weight is that of the rotated
        basis and the forward rotates x first."""
        m, n = _shapes_mx(qweight, scales)
        extras = cls._extras_args(m, n, bias, lowrank, rotation)
        dev = device if device is not None else qweight.device
        q = cls(n, m, device=dev, act_format=act_format, **extras)
        return q._fill(dict(qweight=qweight, scales=scales), bias, lowrank, rotation)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, "
                f"format=mxfp4, bias={self.bias is not None}, act_format={self.act_format}"
                f"{self._extras_repr()}")

    def _dense(self, dtype: torch.dtype) -> torch.Tensor:
        return dequantize_packed_mx(self.qweight, self.scales, dtype)

    def _gemm(self, x2: torch.Tensor, T: int, ldx: int, bias: Optional[torch.Tensor],
              out: torch.Tensor) -> None:
        n, m = self.in_features, self.out_features
        if self.act_format is not None:
            nbytes = lib.tg_qgemm_mx_act_workspace_size(T, m, n)
            ws = workspace(nbytes, x2.device)
            call("tg_qgemm_mx_act", stream(), ptr(x2), DTYPES[x2.dtype], T, ldx,
                 ptr(self.qweight), ptr(self.scales), TG_FMT_MXFP4,
                 ACT_FORMATS[self.act_format], m, n, ptr(bias),
                 DTYPES[bias.dtype] if bias is not None else 0, ptr(out), DTYPES[out.dtype],
                 m, ptr(ws), nbytes)
        else:
            nbytes = lib.tg_qgemm_workspace_size(T, m, n)
            ws = workspace(nbytes, x2.device)
            call("tg_qgemm_mx", stream(), ptr(x2), DTYPES[x2.dtype], T, ldx, ptr(self.qweight),
                 ptr(self.scales), TG_FMT_MXFP4, m, n, ptr(bias),
                 DTYPES[bias.dtype] if bias is not None else 0, ptr(out), DTYPES[out.dtype], m,
                 ptr(ws), nbytes)


# ---------------------------------------------------------------------------
# Mixture of Experts (A19)
# ---------------------------------------------------------------------------
def qgemm_grouped(x: torch.Tensor, rows: Optional[torch.Tensor], offsets: torch.Tensor,
                  qweight: torch.Tensor, qzeros: Optional[torch.Tensor], scales: torch.Tensor,
                  w_bits: int, group_size: int, row_scale: Optional[torch.Tensor] = None,
                  dtype: Optional[torch.dtype] = None, act_format=None) -> torch.Tensor:
    """``Y[i] = row_scale[i] * x[rows[i]] @ W^_e^T`` for every slot i of expert e,
    ``offsets[e] <= i < offsets[e + 1]`` (``tg_qgemm_grouped``).  x (T, n) fp16 /
    bf16; rows int32 (R,) or None (slot i reads row i); offsets int32 (E + 1,);
    qweight (E, n*b/32, m) with qzeros (E, G, m*b/32) and scales (E, G, m), or
    ``qzeros=None`` with uint8 scales (E, n/32, m) for MXFP4; row_scale fp32 (R,)
    or None.  Returns (R, m) of `dtype` (x's, or float32).  Everything stays on
    the device: nothing is read back.  ``act_format="mxfp8"`` (MXFP4 stacks only):
    every row of x is quantised to MXFP8 once and both operands go to the
    block-scaled MFMA as they lie in memory (``tg_qgemm_grouped_act``)."""
    _check_act_format(act_format, ACT_FORMATS, " for qgemm_grouped")
    if act_format is not None and qzeros is not None:
        raise ValueError(f"qgemm_grouped: act_format={act_format!r} needs MXFP4 stacks "
                         "(qzeros=None, uint8 scales); integer stacks take 16-bit activations")
    require_cuda(x, "qgemm_grouped input")
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError(f"qgemm_grouped takes float16 or bfloat16 activations, got {x.dtype} "
                           "(there is no fp32 kernel and no fallback)")
    E, nw, m = qweight.shape
    mx = qzeros is None
    n = nw * 32 // w_bits
    T = x.shape[0]
    R = T if rows is None else rows.numel()
    dtype = x.dtype if dtype is None else dtype
    if x.dim() != 2 or x.shape[1] != n:
        raise ValueError(f"qgemm_grouped: x must be (T, {n}) for this qweight, got {tuple(x.shape)}")
    for what, t, dt, numel in (("rows", rows, torch.int32, R), ("offsets", offsets, torch.int32, E + 1),
                               ("row_scale", row_scale, torch.float32, R)):
        if t is not None and (t.dtype != dt or t.device != x.device or t.numel() != numel
                              or not t.is_contiguous()):
            raise ValueError(f"qgemm_grouped: {what} must be a contiguous {dt} tensor of {numel} "
                             f"elements on {x.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    y = torch.empty((R, m), dtype=dtype, device=x.device)
    if R == 0:
        return y
    x, T, ldx = _rows(x, n)
    with torch.cuda.device(x.device):
        if act_format is not None:
            nbytes = lib.tg_qgemm_grouped_act_workspace_size(T, R, E, m, n)
            ws = workspace(nbytes, x.device)
            call("tg_qgemm_grouped_act", stream(), ptr(x), DTYPES[x.dtype], T, ldx, ptr(rows),
                 ptr(offsets), R, E, ptr(qweight), ptr(scales), TG_FMT_MXFP4,
                 ACT_FORMATS[act_format], m, n, ptr(row_scale), ptr(y), DTYPES[dtype], m, ptr(ws),
                 nbytes)
            return y
        nbytes = lib.tg_qgemm_grouped_workspace_size(R, E, m, n)
        ws = workspace(nbytes, x.device)
        call("tg_qgemm_grouped", stream(), ptr(x), DTYPES[x.dtype], T, ldx, ptr(rows), ptr(offsets),
             R, E, ptr(qweight), ptr(qzeros), ptr(scales), 0 if mx else DTYPES[scales.dtype],
             TG_FMT_MXFP4 if mx else 0, m, n, 32 if mx else group_size, w_bits, ptr(row_scale),
             ptr(y), DTYPES[dtype], m, ptr(ws), nbytes)
    return y


class QuantExperts(nn.Module):
    """A layer's experts with both weight stacks packed: the drop-in for a module
    with ``gate_up_proj`` (E, 2I, H), ``down_proj`` (E, H, I) and
    ``forward(hidden_states, top_k_index, top_k_weights)``.  Buffers (the
    checkpoint's keys): ``gate_up_qweight`` (E, H*b/32, 2I), ``gate_up_qzeros``
    (E, G, 2I*b/32), ``gate_up_scales`` (E, G, 2I) and the same three for ``down``
    with H and I exchanged; every ``[e]`` is what ``pack_quantized`` returns for
    that expert.  ``weight_format="mxfp4"``: no ``qzeros``, uint8 ``scales``
    (E, in/32, out), bits 4 and group 32.  There is no bias.
    ``act_format`` (a plain attribute, not in the ``state_dict``): None, 16-bit
    activations; "mxfp8", for ``weight_format="mxfp4"``: both grouped calls
    quantise their input to MXFP8 and run on the block-scaled MFMA
    (``qgemm_grouped(act_format="mxfp8")``); the SwiGLU between them stays 16-bit."""

    def __init__(self, num_experts: int, hidden_dim: int, intermediate_dim: int, w_bits: int = 4,
                 group_size: int = -1, weight_format: str = "int",
                 scale_dtype: torch.dtype = torch.float16, act_fn=None, device=None,
                 act_format=None):
        super().__init__()
        if weight_format not in ("int", "mxfp4"):
            raise ValueError(f"weight_format must be 'int' or 'mxfp4', got {weight_format!r}")
        _check_act_format(act_format, ACT_FORMATS, " for QuantExperts")
        if act_format is not None and weight_format != "mxfp4":
            raise ValueError(f"act_format={act_format!r} needs weight_format='mxfp4', got "
                             f"{weight_format!r}")
        self.act_format = act_format
        mx = weight_format == "mxfp4"
        if mx:
            w_bits, group_size = 4, 32
        if w_bits not in _BITS:
            raise ValueError(f"w_bits must be one of {_BITS}, got {w_bits}")
        E, H, I = int(num_experts), int(hidden_dim), int(intermediate_dim)
        if not 1 <= E <= 256:
            raise ValueError(f"QuantExperts takes 1 to 256 experts, got {E}")
        for n_in, n_out in ((H, 2 * I), (I, H)):
            g = group_size if group_size > 0 else n_in
            if n_in % 32 or g % 32 or n_in % g or (n_out * w_bits) % 32:
                raise ValueError(
                    f"QuantExperts needs in % 32 == 0, group % 32 == 0 dividing in and out * bits "
                    f"% 32 == 0 for both stacks (got hidden={H}, intermediate={I}, "
                    f"group={group_size}, bits={w_bits})")
        self.num_experts, self.hidden_dim, self.intermediate_dim = E, H, I
        self.w_bits, self.group_size, self.weight_format = int(w_bits), int(group_size), weight_format
        self.act_fn = act_fn if act_fn is not None else nn.functional.silu
        for name, n_in, n_out in (("gate_up", H, 2 * I), ("down", I, H)):
            G = n_in // (group_size if group_size > 0 else n_in)
            self.register_buffer(f"{name}_qweight", torch.zeros((E, n_in * w_bits // 32, n_out),
                                                                dtype=torch.int32, device=device))
            if mx:
                setattr(self, f"{name}_qzeros", None)
                self.register_buffer(f"{name}_scales", torch.full((E, G, n_out), 127,
                                                                  dtype=torch.uint8, device=device))
            else:
                self.register_buffer(f"{name}_qzeros", torch.zeros((E, G, n_out * w_bits // 32),
                                                                   dtype=torch.int32, device=device))
                self.register_buffer(f"{name}_scales", torch.zeros((E, G, n_out), dtype=scale_dtype,
                                                                   device=device))

    @classmethod
    def from_packed(cls, gate_up: dict, down: dict, w_bits: int = 4, group_size: int = -1,
                    weight_format: str = "int", act_fn=None, device=None,
                    act_format=None) -> "QuantExperts":
        """From the two stacked entries (a checkpoint's, or ``quantize_model``'s
        ``packed``): dicts of ``qweight`` (E, in*b/32, out), ``qzeros`` (None for
        MXFP4) and ``scales``."""
        if weight_format == "mxfp4":
            w_bits = 4
        E, nw, m2 = gate_up["qweight"].shape
        H, I = nw * 32 // w_bits, m2 // 2
        dev = device if device is not None else gate_up["qweight"].device
        q = cls(E, H, I, w_bits, group_size, weight_format, scale_dtype=gate_up["scales"].dtype
                if weight_format == "int" else torch.float16, act_fn=act_fn, device=dev,
                act_format=act_format)
        for name, t in (("gate_up", gate_up), ("down", down)):
            for k in ("qweight", "qzeros", "scales"):
                buf = getattr(q, f"{name}_{k}")
                if buf is None:
                    continue
                if t.get(k) is None or tuple(t[k].shape) != tuple(buf.shape) \
                        or t[k].dtype != buf.dtype:
                    raise ValueError(f"{name}.{k}: expected {buf.dtype} {tuple(buf.shape)}, got "
                                     f"{None if t.get(k) is None else (t[k].dtype, tuple(t[k].shape))}")
                buf.copy_(t[k])
        return q

    def extra_repr(self) -> str:
        fmt = "format=mxfp4" if self.weight_format == "mxfp4" else \
            f"bits={self.w_bits}, group_size={self.group_size}"
        act = f", act_format={self.act_format}" if self.act_format is not None else ""
        return (f"num_experts={self.num_experts}, hidden_dim={self.hidden_dim}, "
                f"intermediate_dim={self.intermediate_dim}, {fmt}{act}")

    def dequantize(self, dtype: torch.dtype = torch.float16):
        """The dense ``(gate_up_proj (E, 2I, H), down_proj (E, H, I))`` of `dtype`."""
        out = []
        for name in ("gate_up", "down"):
            qw, qz, sc = (getattr(self, f"{name}_{k}") for k in ("qweight", "qzeros", "scales"))
            out.append(torch.stack([
                dequantize_packed_mx(qw[e], sc[e], dtype) if qz is None else
                dequantize_packed(qw[e], qz[e], sc[e], self.w_bits, self.group_size, dtype)
                for e in range(self.num_experts)]))
        return tuple(out)

    @torch.no_grad()
    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor,
                top_k_weights: torch.Tensor) -> torch.Tensor:
        require_cuda(hidden_states, "QuantExperts input")
        H, I = self.hidden_dim, self.intermediate_dim
        x = hidden_states.reshape(-1, H)
        T = x.shape[0]
        assert top_k_index.dim() == 2 and top_k_index.shape[0] == T \
            and top_k_weights.shape == top_k_index.shape, "routing tensors must be (tokens, top_k)"
        k = top_k_index.shape[1]
        # assignment a = token * k + choice; slots are the assignments in expert order
        flat = top_k_index.reshape(-1)
        order = torch.argsort(flat, stable=True)
        rows = torch.div(order, k, rounding_mode="floor").to(torch.int32)
        # offsets[e] = number of assignments to experts below e.  (bincount + cumsum
        # would give the same, but bincount on the device sizes its output from the
        # data and so waits for it; searchsorted does not.)
        offsets = torch.searchsorted(flat[order], torch.arange(
            self.num_experts + 1, device=flat.device, dtype=flat.dtype)).to(torch.int32)
        gu = qgemm_grouped(x, rows, offsets, self.gate_up_qweight, self.gate_up_qzeros,
                           self.gate_up_scales, self.w_bits, self.group_size,
                           act_format=self.act_format)
        h = self.act_fn(gu[:, :I]) * gu[:, I:]
        scale = top_k_weights.reshape(-1)[order].to(torch.float32)
        d = qgemm_grouped(h, None, offsets, self.down_qweight, self.down_qzeros, self.down_scales,
                          self.w_bits, self.group_size, row_scale=scale,
                          act_format=self.act_format)
        # token t's k slots through the inverse permutation, added in fp32 in choice
        # order and rounded once (index_add_ would use atomics)
        slot = torch.empty_like(order)
        slot[order] = torch.arange(order.numel(), device=order.device)
        d = d[slot].view(T, k, H)
        acc = d[:, 0].to(torch.float32)
        for j in range(1, k):
            acc += d[:, j]
        return acc.to(hidden_states.dtype).reshape(hidden_states.shape)
