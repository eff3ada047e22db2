"""Packed-weight inference (A14): the consumer of the checkpoint that
``export.save_quantized`` writes.

``dequantize_packed`` decodes the AutoGPTQ ``gptq_v2`` tensors back into the
dense weight (``tg_dequant_packed``); ``QuantLinear`` keeps them packed and
runs ``y = x W^T + bias`` straight from the packed words (``tg_qgemm``: a
split-K GEMV for up to 16 rows, an MFMA tile kernel above).  Both are HIP
kernels; there is no CPU or eager fallback.

Layout (export.py): ``qweight`` int32 (in*b/32, out), ``qzeros`` int32
(G, out*b/32), ``scales`` fp16 or fp32 (G, out), ``g_idx`` int32 (in,) -- only
the trivial map ``arange(in) // group`` (static groups, original column
order).  w = (code_u - zero_u) * scale.

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
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from ._lib import (ACT_FORMATS, DTYPES, TG_FMT_MXFP4, call, lib, ptr, require_cuda, stream,
                   workspace)

__all__ = ["QuantLinear", "dequantize_packed", "MXQuantLinear", "dequantize_packed_mx",
           "quantize_act_mx", "dequantize_act_mx", "add_lowrank", "hadamard"]

_BITS = (2, 3, 4, 8)


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


def dequantize_packed(qweight: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor,
                      w_bits: int, group_size: int,
                      dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """Dense weight (out, in) of `dtype` (fp16 / bf16 / fp32):
    ``float(code_u - zero_u) * float(scale)`` rounded once to `dtype`."""
    m, n, g = _shapes(qweight, qzeros, scales, w_bits, group_size)
    for t, what in ((qweight, "qweight"), (qzeros, "qzeros"), (scales, "scales")):
        require_cuda(t, what)
    if dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise ValueError(f"dtype must be float16, bfloat16 or float32, got {dtype}")
    dev = qweight.device
    qweight, qzeros, scales = qweight.contiguous(), qzeros.contiguous(), scales.contiguous()
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
    x2 = x.reshape(-1, n)
    T = x2.shape[0]
    y = torch.empty((T, n), dtype=dtype, device=x.device)
    if T > 0:
        if x2.stride(1) != 1 or (T > 1 and x2.stride(0) < n):
            x2 = x2.contiguous()
        ldx = x2.stride(0) if T > 1 else n
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


def _register_rotation(mod: nn.Module, block: int, device) -> None:
    """``rotate_block`` and the buffer ``had_sign`` (int32, in/32 words) for
    block > 0; the attribute is None otherwise, like an absent bias."""
    mod.rotate_block = int(block)
    if mod.rotate_block:
        _check_block(block, mod.in_features)
        mod.register_buffer("had_sign", torch.zeros(mod.in_features // 32, dtype=torch.int32,
                                                    device=device))
    else:
        mod.had_sign = None


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


def _register_lowrank(mod: nn.Module, rank: int, dtype: torch.dtype, device) -> None:
    """Buffers ``lr_a`` (out, r), ``lr_b`` (r, in) for rank > 0; the attributes
    are None otherwise, like an absent bias."""
    if rank:
        if not 1 <= rank <= 128:
            raise ValueError(f"lowrank must be in [0, 128], got {rank}")
        if dtype not in _LR_DTYPES:
            raise ValueError("lowrank_dtype must be float16, bfloat16 or float32")
        mod.register_buffer("lr_a", torch.zeros((mod.out_features, rank), dtype=dtype,
                                                device=device))
        mod.register_buffer("lr_b", torch.zeros((rank, mod.in_features), dtype=dtype,
                                                device=device))
    else:
        mod.lr_a = mod.lr_b = None


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


class QuantLinear(nn.Module):
    """A linear layer whose weight stays packed.  The buffer names are the
    checkpoint's keys, so ``load_state_dict`` fills it.  ``module.to(dtype)``
    converts floating buffers like any module: fp32 ``scales`` become 16-bit
    with it (and the decoded weight changes accordingly)."""

    def __init__(self, in_features: int, out_features: int, w_bits: int, group_size: int,
                 bias: bool = False, scale_dtype: torch.dtype = torch.float16,
                 bias_dtype: torch.dtype = torch.float16, device=None, lowrank: int = 0,
                 lowrank_dtype: torch.dtype = torch.float16, rotate_block: int = 0):
        super().__init__()
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
        if bias:
            self.register_buffer("bias", torch.zeros(out_features, dtype=bias_dtype, device=device))
        else:
            self.bias = None
        _register_lowrank(self, int(lowrank), lowrank_dtype, device)
        _register_rotation(self, rotate_block, device)

    @classmethod
    def from_packed(cls, qweight: torch.Tensor, qzeros: torch.Tensor, scales: torch.Tensor,
                    w_bits: int, group_size: int, bias: Optional[torch.Tensor] = None,
                    g_idx: Optional[torch.Tensor] = None, device=None,
                    lowrank=None, rotation=None) -> "QuantLinear":
        """From the packed tensors (a checkpoint's, or ``pack_quantized``'s).
        `g_idx`, when given, must be the trivial ``arange(in) // group``.
        ``lowrank=(A, B)``: the correction's factors, (out, r) and (r, in).
        ``rotation=(block, sign_bits)``: the packed weight is that of the rotated
        basis and the forward rotates x first."""
        m, n, g = _shapes(qweight, qzeros, scales, w_bits, group_size)
        if lowrank is not None:
            lowrank = _check_lowrank(lowrank, m, n)
        if rotation is not None:
            rotation = _check_rotation(rotation, n)
        if g_idx is not None:
            triv = torch.arange(n, dtype=torch.int64) // g
            if tuple(g_idx.shape) != (n,) or not torch.equal(g_idx.cpu().to(torch.int64), triv):
                raise ValueError("g_idx is not the static arange(in_features) // group_size map "
                                 "(act-order checkpoints are not supported)")
        dev = device if device is not None else qweight.device
        q = cls(n, m, w_bits, group_size, bias=bias is not None, scale_dtype=scales.dtype,
                bias_dtype=bias.dtype if bias is not None else torch.float16, device=dev,
                lowrank=lowrank[0].shape[1] if lowrank is not None else 0,
                lowrank_dtype=lowrank[0].dtype if lowrank is not None else torch.float16,
                rotate_block=rotation[0] if rotation is not None else 0)
        q.qweight.copy_(qweight)
        q.qzeros.copy_(qzeros)
        q.scales.copy_(scales)
        if bias is not None:
            q.bias.copy_(bias.detach())
        if lowrank is not None:
            q.lr_a.copy_(lowrank[0].detach())
            q.lr_b.copy_(lowrank[1].detach())
        if rotation is not None:
            q.had_sign.copy_(rotation[1])
        return q

    def extra_repr(self) -> str:
        lr = f", lowrank={self.lr_a.shape[1]}" if self.lr_a is not None else ""
        if self.rotate_block:
            lr += f", rotate_block={self.rotate_block}"
        return (f"in_features={self.in_features}, out_features={self.out_features}, "
                f"bits={self.w_bits}, group_size={self.group_size}, "
                f"bias={self.bias is not None}{lr}")

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
            W = dequantize_packed(self.qweight, self.qzeros, self.scales, self.w_bits,
                                  self.group_size, torch.float32)
            W = add_lowrank(W, self.lr_a, self.lr_b, dt)
        else:
            W = dequantize_packed(self.qweight, self.qzeros, self.scales, self.w_bits,
                                  self.group_size, dt)
        return hadamard(W, self.rotate_block, self.had_sign, inverse=True, dtype=dtype) \
            if back else W

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        require_cuda(x, "QuantLinear input")
        require_cuda(self.qweight, "QuantLinear.qweight")
        if x.dtype not in (torch.float16, torch.bfloat16):
            raise RuntimeError(f"QuantLinear takes float16 or bfloat16 activations, got {x.dtype} "
                               "(there is no fp32 kernel and no fallback)")
        if x.shape[-1] != self.in_features:
            raise RuntimeError(f"QuantLinear: last dim {x.shape[-1]} != in_features "
                               f"{self.in_features}")
        n, m = self.in_features, self.out_features
        x2 = x.reshape(-1, n)
        T = x2.shape[0]
        y = torch.empty((T, m), dtype=x.dtype, device=x.device)
        if T > 0:
            if x2.stride(1) != 1 or (T > 1 and x2.stride(0) < n):
                x2 = x2.contiguous()
            ldx = x2.stride(0) if T > 1 else n
            if self.rotate_block:
                x2, ldx = _rotate_rows(x2, T, n, ldx, self.rotate_block, self.had_sign), n
            bias = self.bias
            lr = self.lr_a is not None
            # with a correction the GEMM leaves its fp32 sums; tg_lr_finish adds the bias
            out = torch.empty((T, m), dtype=torch.float32, device=x.device) if lr else y
            gb = None if lr else bias
            with torch.cuda.device(x.device):
                nbytes = lib.tg_qgemm_workspace_size(T, m, n)
                ws = workspace(nbytes, x.device)
                call("tg_qgemm", stream(), ptr(x2), DTYPES[x.dtype], T, ldx, ptr(self.qweight),
                     ptr(self.qzeros), ptr(self.scales), DTYPES[self.scales.dtype], m, n,
                     self.group_size, self.w_bits, ptr(gb),
                     DTYPES[gb.dtype] if gb is not None else 0, ptr(out), DTYPES[out.dtype], m,
                     ptr(ws), nbytes)
                if lr:
                    _lowrank_finish(x2, T, ldx, out, self.lr_a, self.lr_b, bias, y)
        return y.reshape(*x.shape[:-1], m)


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


def _check_act_format(act_format) -> None:
    if act_format is not None and (not isinstance(act_format, str)
                                   or act_format not in ACT_FORMATS):
        raise ValueError(f"act_format must be None or one of {sorted(ACT_FORMATS)}, got "
                         f"{act_format!r}")


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
    x2 = x.reshape(-1, n)
    T = x2.shape[0]
    xq = torch.empty((T, n), dtype=torch.uint8, device=x.device)
    xs = torch.empty((T, n // 32), dtype=torch.uint8, device=x.device)
    if T > 0:
        if x2.stride(1) != 1 or (T > 1 and x2.stride(0) < n):
            x2 = x2.contiguous()
        ldx = x2.stride(0) if T > 1 else n
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


class MXQuantLinear(nn.Module):
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
        _check_act_format(act_format)
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
        if bias:
            self.register_buffer("bias", torch.zeros(out_features, dtype=bias_dtype, device=device))
        else:
            self.bias = None
        _register_lowrank(self, int(lowrank), lowrank_dtype, device)
        _register_rotation(self, rotate_block, device)

    @classmethod
    def from_packed(cls, qweight: torch.Tensor, scales: torch.Tensor,
                    bias: Optional[torch.Tensor] = None, device=None,
                    act_format=None, lowrank=None, rotation=None) -> "MXQuantLinear":
        """From the packed pair (a checkpoint's, or ``pack_quantized``'s).
        ``lowrank=(A, B)``: the correction's factors, (out, r) and (r, in).
        ``rotation=(block, sign_bits)``: the packed weight is that of the rotated
        basis and the forward rotates x first."""
        m, n = _shapes_mx(qweight, scales)
        if lowrank is not None:
            lowrank = _check_lowrank(lowrank, m, n)
        if rotation is not None:
            rotation = _check_rotation(rotation, n)
        dev = device if device is not None else qweight.device
        q = cls(n, m, bias=bias is not None,
                bias_dtype=bias.dtype if bias is not None else torch.float16, device=dev,
                act_format=act_format,
                lowrank=lowrank[0].shape[1] if lowrank is not None else 0,
                lowrank_dtype=lowrank[0].dtype if lowrank is not None else torch.float16,
                rotate_block=rotation[0] if rotation is not None else 0)
        q.qweight.copy_(qweight)
        q.scales.copy_(scales)
        if bias is not None:
            q.bias.copy_(bias.detach())
        if lowrank is not None:
            q.lr_a.copy_(lowrank[0].detach())
            q.lr_b.copy_(lowrank[1].detach())
        if rotation is not None:
            q.had_sign.copy_(rotation[1])
        return q

    def extra_repr(self) -> str:
        lr = f", lowrank={self.lr_a.shape[1]}" if self.lr_a is not None else ""
        if self.rotate_block:
            lr += f", rotate_block={self.rotate_block}"
        return (f"in_features={self.in_features}, out_features={self.out_features}, "
                f"format=mxfp4, bias={self.bias is not None}, act_format={self.act_format}{lr}")

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
            W = add_lowrank(dequantize_packed_mx(self.qweight, self.scales, torch.float32),
                            self.lr_a, self.lr_b, dt)
        else:
            W = dequantize_packed_mx(self.qweight, self.scales, dt)
        return hadamard(W, self.rotate_block, self.had_sign, inverse=True, dtype=dtype) \
            if back else W

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        require_cuda(x, "MXQuantLinear input")
        require_cuda(self.qweight, "MXQuantLinear.qweight")
        if x.dtype not in (torch.float16, torch.bfloat16):
            raise RuntimeError(f"MXQuantLinear takes float16 or bfloat16 activations, got "
                               f"{x.dtype} (there is no fp32 kernel and no fallback)")
        if x.shape[-1] != self.in_features:
            raise RuntimeError(f"MXQuantLinear: last dim {x.shape[-1]} != in_features "
                               f"{self.in_features}")
        n, m = self.in_features, self.out_features
        x2 = x.reshape(-1, n)
        T = x2.shape[0]
        y = torch.empty((T, m), dtype=x.dtype, device=x.device)
        if T > 0:
            if x2.stride(1) != 1 or (T > 1 and x2.stride(0) < n):
                x2 = x2.contiguous()
            ldx = x2.stride(0) if T > 1 else n
            if self.rotate_block:
                x2, ldx = _rotate_rows(x2, T, n, ldx, self.rotate_block, self.had_sign), n
            bias = self.bias
            lr = self.lr_a is not None
            # with a correction the GEMM leaves its fp32 sums; tg_lr_finish adds the bias.
            # Z = x lr_b^T always comes from the 16-bit x, under act_format too.
            out = torch.empty((T, m), dtype=torch.float32, device=x.device) if lr else y
            gb = None if lr else bias
            if self.act_format is not None:
                with torch.cuda.device(x.device):
                    nbytes = lib.tg_qgemm_mx_act_workspace_size(T, m, n)
                    ws = workspace(nbytes, x.device)
                    call("tg_qgemm_mx_act", stream(), ptr(x2), DTYPES[x.dtype], T, ldx,
                         ptr(self.qweight), ptr(self.scales), TG_FMT_MXFP4,
                         ACT_FORMATS[self.act_format], m, n, ptr(gb),
                         DTYPES[gb.dtype] if gb is not None else 0, ptr(out), DTYPES[out.dtype],
                         m, ptr(ws), nbytes)
                    if lr:
                        _lowrank_finish(x2, T, ldx, out, self.lr_a, self.lr_b, bias, y)
                return y.reshape(*x.shape[:-1], m)
            with torch.cuda.device(x.device):
                nbytes = lib.tg_qgemm_workspace_size(T, m, n)
                ws = workspace(nbytes, x.device)
                call("tg_qgemm_mx", stream(), ptr(x2), DTYPES[x.dtype], T, ldx, ptr(self.qweight),
                     ptr(self.scales), TG_FMT_MXFP4, m, n, ptr(gb),
                     DTYPES[gb.dtype] if gb is not None else 0, ptr(out), DTYPES[out.dtype], m,
                     ptr(ws), nbytes)
                if lr:
                    _lowrank_finish(x2, T, ldx, out, self.lr_a, self.lr_b, bias, y)
        return y.reshape(*x.shape[:-1], m)
