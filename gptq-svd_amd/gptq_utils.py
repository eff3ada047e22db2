"""Drop-in counterpart of the reference solver API on MI355X.

Mirrors the names, argument meaning and error behaviour of
``/root/reference/src/TruncGPTQ/gptq_utils.py`` so the layer-sequential harness
(``quantize.py:14``) only has to change its import line:

    from gptq_svd_amd.gptq_utils import (gptq_fwrd, Quantizer, process_hessian_alt,
                                         HessianAccumulator, Sketcher, process_sketch)

Every numerical stage runs in the HIP library (``libtruncgptq.so``, C ABI in
``include/truncgptq.h``) on the caller's current HIP stream; torch provides
device memory, streams and the caching allocator only.  There is no CPU
fallback: CPU tensors raise ``RuntimeError``.
"""
from __future__ import annotations

import ctypes
import logging
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream, workspace

__all__ = [
    "HessianAccumulator", "process_hessian_alt", "process_hessian", "Quantizer", "gptq_fwrd",
    "triton_process_block", "log_quantization_error", "next_power_of_2",
    "truncated_spectral_factor", "pack_quantized", "Sketcher", "process_sketch",
    "lowrank_correction", "HadamardRotation",
]


# ---------------------------------------------------------------------------
# A1  (gptq_utils.py:213-228)
# ---------------------------------------------------------------------------
class HessianAccumulator:
    """H += x^T x in float64 (FP64 MFMA SYRK kernel; fp16 / bf16 inputs take
    the dedicated 16-bit SYRK of syrk.hip); get_hessian() = H / N."""

    def __init__(self, in_features, device, dtype=torch.float64):
        if dtype != torch.float64:
            raise RuntimeError("HessianAccumulator: only float64 accumulation is supported")
        self.H = torch.zeros((in_features, in_features), device=device, dtype=dtype)
        _lib.require_cuda(self.H, "HessianAccumulator device")
        self.n_samples = 0
        self._ws = None

    def add_batch(self, x):                                   # gptq_utils.py:218-223
        if x.dim() == 3:
            x = x.reshape(-1, x.shape[-1])
        _lib.require_cuda(x, "add_batch input")
        if x.dtype not in _lib.DTYPES:
            x = x.to(torch.float64)
        if x.stride(-1) != 1:
            x = x.contiguous()
        rows, n = x.shape
        if n != self.H.shape[0]:
            raise RuntimeError(f"add_batch: expected {self.H.shape[0]} features, got {n}")
        if rows:
            with torch.cuda.device(self.H.device):
                # the 16-bit SYRK's partial-tile scratch, only for inputs that
                # take it (fp16 / bf16, n and the row stride multiples of 8,
                # 16-byte aligned); everything else runs the generic path
                b16 = (x.dtype in (torch.float16, torch.bfloat16) and n % 8 == 0
                       and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0)
                if b16 and self._ws is None:
                    self._ws = workspace(_lib.lib.tg_syrk_workspace_size(n), self.H.device)
                if b16:
                    call("tg_syrk_accum_ws", stream(), ptr(x), _lib.DTYPES[x.dtype], rows, n,
                         x.stride(0), ptr(self.H), self.H.shape[0], ptr(self._ws),
                         self._ws.numel())
                else:
                    call("tg_syrk_accum", stream(), ptr(x), _lib.DTYPES[x.dtype], rows, n,
                         x.stride(0), ptr(self.H), self.H.shape[0])
        self.n_samples += rows

    def get_hessian(self):                                    # gptq_utils.py:225-228
        if self.n_samples == 0:
            return self.H
        out = torch.empty_like(self.H)
        with torch.cuda.device(self.H.device):
            call("tg_scale_f64", stream(), ptr(self.H), self.H.numel(),
                 -float(self.n_samples), ptr(out))
        return out


# ---------------------------------------------------------------------------
# A2-A5  (gptq_utils.py:87-126)
# ---------------------------------------------------------------------------
class SpectrumSplit(NamedTuple):
    """What the complement path needs to know about the dropped spectrum."""
    nc: int          # dropped eigenvalues above the rounding threshold tau = n*eps*lambda_max
    lam_k: float     # smallest kept eigenvalue
    psd: bool        # every dropped eigenvalue >= -tau
    left: float      # max |lambda| of the dropped eigenvalues at or below tau


def _complement_count(w_asc, k: int) -> SpectrumSplit:
    """Split of the ascending spectrum at rank k (a device tensor: one 8n-byte
    copy; or a host numpy array).  numpy on the host copy: a handful of torch
    CPU ops cost ~0.3 ms of host time between two GPU phases."""
    w = w_asc.double().cpu().numpy() if isinstance(w_asc, torch.Tensor) else np.asarray(w_asc)
    n = w.shape[0]
    tau = n * 2.220446049250313e-16 * max(float(w[-1]), 0.0)
    dropped = w[:n - k]
    low = dropped[dropped <= tau]
    return SpectrumSplit(int(np.count_nonzero(dropped > tau)), float(w[n - k]),
                         bool(float(w[0]) >= -tau),
                         float(np.abs(low).max()) if low.size else 0.0)


def spectral_path(n: int, k: int, sp: SpectrumSplit) -> str:
    """'complement' when the dropped eigenpairs that matter are fewer than
    the kept ones (k > n/2 in practice) and the complement form is exact to
    ~1e-9: no kept eigenvalue is clamped by sqrt(max(L, 1e-12))
    (gptq_utils.py:94); no dropped eigenvalue is below -tau; and the dropped
    eigenvalues H_k = H - B_c^T B_c keeps (those at or below tau) are below
    1e-9 lambda_k, since they perturb the pseudo-inverse by ~left / lambda_k
    (graded spectra reaching down to rounding level fail this, the kept path
    is exact for them).  Else 'kept'.  TG_SPECTRAL_PATH = kept | complement
    forces one (complement only where it is defined)."""
    import os
    force = os.environ.get("TG_SPECTRAL_PATH", "auto")
    defined = sp.lam_k >= 1e-12 and sp.nc <= k and k + sp.nc <= n and sp.psd
    if force == "kept" or not defined:
        return "kept"
    if force == "complement":
        return "complement"
    exact = sp.left <= 1e-9 * sp.lam_k
    return "complement" if sp.nc < k and exact else "kept"


# tg_u_factor_last_path() -> truncated_spectral_factor.last_ufactor
_UFACTOR_PATHS = ("gram", "refined", "householder")


def truncated_spectral_factor(H: torch.Tensor, threshold: float = 0.0005,
                              threshold_method: str = "mean_trimmed", want_rx: bool = True,
                              min_rank: int = 0):
    """Native pipeline behind process_hessian_alt.  Returns (U, R_x, perm, S, k).

    eigh (two-stage reduction + bisection) -> rank rule -> then either
      kept path:       eigenvectors of the k kept eigenvalues, greedy-pivoted
                       factor of H_k = S_k^T S_k (the dgeqp3 pivot order and
                       R_x), U = R(QR(diag(1/S_k) Vh_k P));
      complement path: eigenvectors of the nc dropped eigenvalues above the
                       rounding threshold only, H_k = H - B_c^T B_c, the same
                       pivoting, U = R(QR(S^-1 R_x)), S = R_x R_x^T
    whichever needs fewer eigenvectors.

    U comes from the Cholesky factor of a Gram matrix; when that form and its
    CholeskyQR refinement break down the library takes it from a Householder
    QR, like the reference (gptq_utils.py:120), and ``last_ufactor`` says so
    ("gram" | "refined" | "householder").  A breakdown of the complement
    path's tg_u_factor_rx reruns the kept path (``last_path[0] == "kept"``).
    ``min_rank`` clamps the rule's rank from below (process_sketch keeps at
    least one direction, gptq_utils.py:65); the default raises on rank 0.
    """
    _lib.require_cuda(H, "process_hessian_alt H")
    n = H.shape[0]
    if H.dim() != 2 or H.shape[1] != n:
        raise RuntimeError("process_hessian_alt: H must be square")
    dev = H.device
    rule = _lib.RULES.get(threshold_method, 0)
    with torch.cuda.device(dev):
        Hd = H.to(dtype=torch.float64).contiguous()
        A = Hd.clone()
        ws = workspace(_lib.lib.tg_eigh_workspace_size(n), dev)
        w = torch.empty(n, dtype=torch.float64, device=dev)
        call("tg_eigh_values", stream(), ptr(A), n, n, ptr(w), ptr(ws), ws.numel())
        S = torch.empty(n, dtype=torch.float64, device=dev)
        kdev = torch.empty(1, dtype=torch.int32, device=dev)
        call("tg_truncation_rank", stream(), ptr(w), n, float(threshold), rule, ptr(S), ptr(kdev))
        # one host sync for the rank and the spectrum split (the reference syncs
        # here too, gptq_utils.py:100, :106)
        wk = torch.cat((w, kdev.to(torch.float64))).cpu().numpy()
        k = max(int(wk[n]), min(int(min_rank), n))
        if k < 1:
            raise RuntimeError("process_hessian_alt: truncation rank is 0 "
                               "(threshold keeps no eigenvalue)")
        del A
        sp = _complement_count(wk[:n], k)
        nc = sp.nc
        path = spectral_path(n, k, sp)
        perm = torch.empty(n, dtype=torch.int64, device=dev)
        R_x = torch.empty((k, n), dtype=torch.float64, device=dev)
        U = torch.empty((k, n), dtype=torch.float64, device=dev)

        def kept_branch():
            nonlocal ws  # the eigensolver workspace is released before the next one is taken
            Vh = torch.empty((k, n), dtype=torch.float64, device=dev)
            call("tg_eigh_vectors", stream(), n, ptr(w), k, ptr(Vh), n, ptr(ws), ws.numel())
            ws = None
            pws = workspace(_lib.lib.tg_pivot_workspace_size(n, k), dev)
            call("tg_pivoted_factor", stream(), ptr(Vh), n, ptr(S), n, k, ptr(perm), ptr(R_x),
                 n, ptr(pws), pws.numel())
            del pws
            uws = workspace(_lib.lib.tg_ufactor_workspace_size(n, k), dev)
            call("tg_u_factor", stream(), ptr(Vh), n, ptr(S), ptr(perm), n, k, ptr(U), n,
                 ptr(uws), uws.numel())

        if path == "kept":
            kept_branch()
        else:
            Vc = torch.empty((max(nc, 1), n), dtype=torch.float64, device=dev)
            if nc:
                call("tg_eigh_vectors_range", stream(), n, ptr(w), k, nc, ptr(Vc), n, ptr(ws),
                     ws.numel())
            ws = None
            pws = workspace(_lib.lib.tg_pivot_workspace_size(n, k), dev)
            call("tg_pivoted_factor_complement", stream(), ptr(Hd), n, ptr(Vc), n,
                 ptr(S[k:]) if nc else None, nc, n, k, ptr(perm), ptr(R_x), n, ptr(pws),
                 pws.numel())
            del pws, Vc
            uws = workspace(_lib.lib.tg_ufactor_rx_workspace_size(n, k), dev)
            try:
                call("tg_u_factor_rx", stream(), ptr(R_x), n, n, k, ptr(U), n, ptr(uws),
                     uws.numel())
            except RuntimeError as err:
                if "broke down" not in str(err):
                    raise
                # The complement form's C = R11^-1 R12 stages have no Householder
                # form: rerun the kept branch from a fresh copy of Hd.  This costs
                # a second eigensolve on a path that was fatal before; keeping
                # the eigensolver workspace alive on every call instead would
                # raise the default path's peak memory.
                logging.warning(" complement-path U factor broke down (%s); rerunning the "
                                "kept path", err)
                del uws
                path = "kept"
                A = Hd.clone()
                ws = workspace(_lib.lib.tg_eigh_workspace_size(n), dev)
                w = torch.empty(n, dtype=torch.float64, device=dev)
                call("tg_eigh_values", stream(), ptr(A), n, n, ptr(w), ptr(ws), ws.numel())
                del A
                kept_branch()
        truncated_spectral_factor.last_path = (path, nc)
        ufac = _UFACTOR_PATHS[_lib.lib.tg_u_factor_last_path()]
        truncated_spectral_factor.last_ufactor = ufac
        if ufac == "householder":
            logging.warning(" U factor: the Gram form broke down or was switched off; "
                            "Householder QR used (n = %d, k = %d)", n, k)
    return U, (R_x if want_rx else None), perm, S, k


# ---------------------------------------------------------------------------
# A1s  sketch mode  (gptq_utils.py:33-84, :171-211)
# ---------------------------------------------------------------------------
class Sketcher:
    """Y += Omega x with a Gaussian Omega (rank x tokens) that is generated
    inside the GEMM kernel and never stored (tg_sketch_accum; the reference
    draws a torch.randn of rank x tokens per hook call and calls addmm_,
    gptq_utils.py:196-200).

    Omega is a pure function of (seed, sketch row, global token index)
    (include/truncgptq.h), so Y does not depend on how the calibration tokens
    are split into batches, and the same seed reproduces Y bit for bit.
    ``seed=None`` draws one 63-bit seed from torch's default CPU generator at
    construction, so ``torch.manual_seed`` governs a run as it does in the
    reference.  fp16 / bf16 / fp32 inputs go straight into the kernel; other
    dtypes are cast to fp32 (the reference casts everything)."""

    def __init__(self, layer, rank: int, device="cuda", seed: Optional[int] = None):
        self.layer = layer
        self.rank = int(rank)
        self.device = device
        self.in_features = layer.in_features
        if self.rank < 1:
            raise ValueError(f"Sketcher: rank must be positive, got {rank}")
        self.Y = torch.zeros((self.rank, self.in_features), device=device, dtype=torch.float32)
        _lib.require_cuda(self.Y, "Sketcher device")
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
        self.seed = int(seed) & (2 ** 64 - 1)
        self.n_samples = 0

    def hook_fn(self, module, input_args, output):            # gptq_utils.py:184-202
        x = input_args[0]
        if x.dim() > 2:
            x = x.reshape(-1, x.shape[-1])
        if x.shape[0] == 0:
            return
        self.add_batch(x)

    def add_batch(self, x):
        """The harness's accumulator interface (HessianAccumulator.add_batch)."""
        if x.dim() > 2:
            x = x.reshape(-1, x.shape[-1])
        _lib.require_cuda(x, "Sketcher input")
        if x.dtype not in (torch.float16, torch.bfloat16, torch.float32):
            x = x.to(torch.float32)
        if x.stride(-1) != 1:
            x = x.contiguous()
        rows, n = x.shape
        if n != self.in_features:
            raise RuntimeError(f"Sketcher: expected {self.in_features} features, got {n}")
        if rows == 0:
            return
        with torch.cuda.device(self.Y.device):
            call("tg_sketch_accum", stream(), ptr(x), _lib.DTYPES[x.dtype], rows, n, x.stride(0),
                 self.seed, self.n_samples, ptr(self.Y), self.rank, self.Y.stride(0))
        self.n_samples += rows

    def get_scaled_sketch(self):                              # gptq_utils.py:204-211
        if self.n_samples == 0:
            return None, None, 0
        self.Y.mul_(1.0 / float(np.sqrt(float(self.n_samples) * float(self.rank))))
        return self.Y


def process_sketch(sketch: torch.Tensor, threshold: float = 1e-2,
                   threshold_method: str = "mean_trimmed"
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(R, perm) like gptq_utils.py:33-84: R float64 k x n upper trapezoidal with
    positive diagonal, perm int64.

    Gram route.  The reference takes the singular values S and right vectors
    Vh of the sketch Y from geqrf followed by svd(R); these are the eigenpairs
    (S^2, Vh) of G = Y^T Y.  Here G is formed in float64 from the fp32 sketch
    (tg_syrk_accum: products and sums in float64) and the eigh pipeline of
    process_hessian_alt does the rest: S = sqrt(max(eigenvalue, 1e-12)), the
    same rank rules on S, the pivot order of diag(S_k) Vh_k and R = R(QR(diag(1/S_k) Vh_k
    P)), with the rank clamped to at least 1 (gptq_utils.py:65).  Squaring
    costs nothing the thresholds keep: a kept singular value is within about
    1e-2 of the reference value S[1:33].mean() (mean_trimmed) or carries part
    of 1 - eps of the energy, so its square stands 1e-4 .. 1e-8 below the
    largest eigenvalue, far above float64 rounding (1e-16 n).  Checked on the
    CPU against the QR + SVD route on four synthetic sketches (ar1 n=256 rank
    512 mean_trimmed 1e-2; lognormal n=256 rank 1024 energy 1e-4; gaussian
    n=384 rank 384 mean_trimmed 1e-2; ar1 n=512 rank 512 from 300 tokens,
    rank-deficient with k=291, energy 1e-4): the same k, an identical perm,
    and R within 4e-14 .. 9e-13 relative.

    One difference from the reference's rules: the pipeline's clamp
    S >= 1e-6 (process_hessian_alt's, gptq_utils.py:94) is absent from the
    reference's process_sketch.  Null or rounding-level directions therefore
    sit at S = 1e-6 here instead of ~1e-7 S[0]; mean_trimmed keeps them where
    the reference drops them only if threshold * S[1:33].mean() < 1e-6, i.e.
    for a scaled sketch of order 1e-4 or smaller at threshold 1e-2 (the
    activations themselves that small), and the energy rule counts 1e-12 per
    such direction.  Sketches of ordinary scale are unaffected: the
    rank-deficient goldens (k = 290 of 512 under energy, k = 150 of 256 under
    mean_trimmed) give the reference's k.

    The reference's CPU round trip of the sketch (:40-46) is memory juggling
    and is not reproduced.  An unknown ``threshold_method`` raises ValueError
    (the reference hits a NameError there)."""
    if threshold_method not in ("energy", "mean_trimmed"):
        raise ValueError(f"process_sketch: unknown threshold_method {threshold_method!r}")
    _lib.require_cuda(sketch, "process_sketch sketch")
    if sketch.dim() != 2:
        raise RuntimeError("process_sketch: the sketch must be rank x in_features")
    Y = sketch.to(torch.float32)
    if Y.stride(-1) != 1:
        Y = Y.contiguous()
    rank, n = Y.shape
    G = torch.zeros((n, n), dtype=torch.float64, device=Y.device)
    with torch.cuda.device(Y.device):
        call("tg_syrk_accum", stream(), ptr(Y), _lib.TG_F32, rank, n, Y.stride(0), ptr(G), n)
    try:
        U, _, perm, _, _ = truncated_spectral_factor(G, threshold, threshold_method,
                                                     want_rx=False, min_rank=1)
    finally:
        del G
    return U, perm


def process_hessian_alt(H: torch.Tensor, threshold: float = 0.0005,
                        threshold_method: str = "mean_trimmed"
                        ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Returns (R, R_x, perm) exactly like gptq_utils.py:87-126:
    R = U (k x n float64, upper trapezoidal, positive diagonal),
    R_x (k x n float64), perm (n int64)."""
    U, R_x, perm, _, _ = truncated_spectral_factor(H, threshold, threshold_method)
    return U, R_x, perm


# ---------------------------------------------------------------------------
# §8(f) GPTQ comparator factor  (gptq_utils.py:129-165)
# ---------------------------------------------------------------------------
def process_hessian(H: torch.Tensor, actorder: bool = False,
                    damp_percent: float = 0.01) -> Tuple[torch.Tensor, torch.Tensor]:
    """(H_inv_chol, perm): upper Cholesky factor of inv(H_p + damp I) with the
    reference's damping ladder damp = 10^e * damp_percent * mean(diag H),
    e = 0..4 (:148-160).  ActOrder: perm = argsort(diag H, descending) (stable
    on ties; the reference's unstable CUDA sort leaves tie order unspecified).
    When every rung fails the factor is the identity -- the reference's
    intent at :162-164, which as written raises NameError (it tests
    `H_inv_chol` but initialises `H_inv_factor`, :147).
    """
    _lib.require_cuda(H, "process_hessian H")
    Hd = H.to(dtype=torch.float64).contiguous()
    n = Hd.shape[0]
    device = Hd.device
    if actorder:
        perm = torch.argsort(torch.diagonal(Hd), descending=True, stable=True)
    else:
        perm = torch.arange(n, device=device)
    R = torch.empty((n, n), dtype=torch.float64, device=device)
    tries = ctypes.c_int(0)
    max_tries = 5
    with torch.cuda.device(device):
        ws = workspace(_lib.lib.tg_hinv_chol_workspace_size(n), device)
        call("tg_hinv_chol", stream(), ptr(Hd), n, n, ptr(perm) if actorder else None,
             float(damp_percent), max_tries, ptr(R), n, ctypes.byref(tries), ptr(ws), ws.numel())
    if tries.value >= max_tries:
        logging.warning(" Hessian is singular. Using Identity fallback.")
    elif tries.value > 0:
        logging.info(f"  Ref-GPTQ required high damping: {10 ** tries.value * damp_percent}")
    return R, perm


# ---------------------------------------------------------------------------
# A7  (gptq_utils.py:230-272)
# ---------------------------------------------------------------------------
class Quantizer:
    """Static-group min/max (asym) or absmax (sym) quantizer; same fields and
    shapes as the reference (scale/zero: (m, n/g, 1) float32).

    ``clip_search=True`` (A7c, new): each group's range is shrunk by the factor
    p = 1 - i / clip_grid, i = 0 .. clip_steps, that minimises the
    round-to-nearest error weighted per column by ``col_weight`` (n values
    >= 0, e.g. diag(H); None = unweighted), the fused search of
    tg_group_params_clip.  i = 0 is the plain min/max (absmax) choice, so the
    weighted error never rises.  ``clip_choice`` (m, n/g int32) and
    ``clip_objective`` (m, n/g, 2 float64: {J_0, J_chosen}) hold the last
    search's results.

    ``weight_format="mxfp4"`` (A15, new): OCP Microscaling FP4 instead of the
    uniform integer grid -- E2M1 elements {0, .5, 1, 1.5, 2, 3, 4, 6} with a
    sign, one power-of-two scale 2^E per 32 columns, E = max(floor(log2 max|w|)
    - 2, -126) (the contract is in include/truncgptq.h).  It needs w_bits = 4
    and group_size = 32 and has no clip search.  ``find_params`` then fills
    ``scale`` (m, n/32, 1) with 2^E, ``zero`` with zeros and ``scale_e8m0``
    (m, n/32) uint8 with the stored bytes E + 127."""

    def __init__(self, w_bits: int = 4, group_size: int = 128, sym: bool = False,
                 clip_search: bool = False, clip_grid: int = 100, clip_steps: int = 80,
                 col_weight: Optional[torch.Tensor] = None, weight_format: str = "int"):
        if weight_format not in ("int", "mxfp4"):
            raise ValueError(f"Quantizer: weight_format must be 'int' or 'mxfp4', got "
                             f"{weight_format!r}")
        if weight_format == "mxfp4":
            if w_bits != 4 or group_size != 32:
                raise ValueError(f"Quantizer: weight_format='mxfp4' needs w_bits=4 and "
                                 f"group_size=32, got w_bits={w_bits}, group_size={group_size}")
            if clip_search:
                raise ValueError("Quantizer: clip_search is not defined for "
                                 "weight_format='mxfp4'")
        self.weight_format = weight_format
        self.scale_e8m0 = None
        self.w_bits = w_bits
        self.group_size = group_size
        self.sym = sym
        if not 0 <= clip_steps < clip_grid:
            raise ValueError(f"Quantizer: need 0 <= clip_steps < clip_grid, got clip_steps="
                             f"{clip_steps}, clip_grid={clip_grid}")
        self.clip_search = bool(clip_search)
        self.clip_grid = int(clip_grid)
        self.clip_steps = int(clip_steps)
        self.col_weight = col_weight
        self.clip_choice = None
        self.clip_objective = None
        if self.sym:
            half_range = 2 ** (w_bits - 1) - 1
            self.max_q = half_range
            self.min_q = -half_range
        else:
            self.max_q = 2 ** w_bits - 1
            self.min_q = 0
        self.scale = None
        self.zero = None

    def find_params(self, weights: torch.Tensor):            # gptq_utils.py:249-266
        _lib.require_cuda(weights, "Quantizer.find_params weights")
        m, n = weights.shape
        g = self.group_size if self.group_size > 0 else n
        assert n % g == 0
        W = weights.to(torch.float32).contiguous()
        G = n // g
        scale = torch.empty((m, G), dtype=torch.float32, device=W.device)
        if self.weight_format == "mxfp4":
            e8m0 = torch.empty((m, G), dtype=torch.uint8, device=W.device)
            with torch.cuda.device(W.device):
                call("tg_group_params_mx", stream(), ptr(W), m, n, n, _lib.TG_FMT_MXFP4,
                     ptr(scale), ptr(e8m0))
            self.scale = scale.unsqueeze(-1)
            self.zero = torch.zeros_like(self.scale)
            self.scale_e8m0 = e8m0
            return
        zero = torch.empty((m, G), dtype=torch.float32, device=W.device)
        if self.clip_search:
            h = self.col_weight
            if h is not None:
                h = torch.as_tensor(h).detach().to(device=W.device, dtype=torch.float32)
                h = h.reshape(-1).clamp_min(0.0).contiguous()
                if h.numel() != n:
                    raise RuntimeError(f"Quantizer.find_params: col_weight has {h.numel()} "
                                       f"entries, the weights have {n} columns")
            choice = torch.empty((m, G), dtype=torch.int32, device=W.device)
            objective = torch.empty((m, G, 2), dtype=torch.float64, device=W.device)
            with torch.cuda.device(W.device):
                call("tg_group_params_clip", stream(), ptr(W), m, n, n, ptr(h), self.group_size,
                     self.w_bits, int(self.sym), self.clip_grid, self.clip_steps, ptr(scale),
                     ptr(zero), ptr(choice), ptr(objective))
            self.clip_choice = choice
            self.clip_objective = objective
        else:
            with torch.cuda.device(W.device):
                call("tg_group_params", stream(), ptr(W), m, n, n, self.group_size, self.w_bits,
                     int(self.sym), ptr(scale), ptr(zero))
        self.scale = scale.unsqueeze(-1)
        self.zero = zero.unsqueeze(-1)

    def get_expanded_params(self, m, n):                       # gptq_utils.py:268-272
        g = self.group_size if self.group_size > 0 else n
        s_expanded = torch.repeat_interleave(self.scale, g, dim=1)
        z_expanded = torch.repeat_interleave(self.zero, g, dim=1)
        return s_expanded[:, :n].squeeze(-1), z_expanded[:, :n].squeeze(-1)


# ---------------------------------------------------------------------------
# A6  (gptq_utils.py:275-291)
# ---------------------------------------------------------------------------
def log_quantization_error(W_orig, W_quant, R_x, perm):
    """||(W_o - W_q) R_x^T||_F / ||W_o R_x^T||_F with W_o = W_orig[:, perm],
    logged in the reference's format (extract_log.py:20 parses it).  Both
    products run in ONE fused FP32 MFMA pass (tg_pred_error: R_x is read as
    float64 and rounded to float32 like the reference's R_x.to(float32), the
    m x k products never leave the chip, their sums of squares are FP64).
    Returns the value (the reference returns None)."""
    if R_x is None or perm is None:
        return None
    _lib.require_cuda(W_orig, "log_quantization_error W_orig")
    dev = W_orig.device
    W = W_orig.to(torch.float32).contiguous()
    Wq = W_quant.to(device=dev, dtype=torch.float32).contiguous()
    R = R_x.to(device=dev, dtype=torch.float64).contiguous()
    p = perm.to(device=dev, dtype=torch.int64).contiguous()
    m, n = W.shape
    k = R.shape[0]
    if Wq.shape != W.shape or R.shape[1] != n or p.numel() != n:
        raise RuntimeError("log_quantization_error: shape mismatch")
    out = torch.empty(2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws = workspace(_lib.lib.tg_pred_error_workspace_size(m, n, k), dev)
        call("tg_pred_error", stream(), ptr(W), ptr(Wq), m, n, n, ptr(R), k, n, ptr(p), ptr(out),
             ptr(ws), ws.numel())
    y_orig_sq, y_diff_sq = out.tolist()  # the reference's .item() sync (:290)
    relative_error = (y_diff_sq ** 0.5) / (y_orig_sq ** 0.5)
    logging.info(f"   [Metric] Relative prediction error: {relative_error:.6f}")
    return relative_error


# ---------------------------------------------------------------------------
# A9  (gptq_utils.py:389-453)
# ---------------------------------------------------------------------------
def next_power_of_2(x: int) -> int:
    return 1 if x == 0 else 2 ** (x - 1).bit_length()


def triton_process_block(w_block, s_block, z_block, R_block, quantizer):
    """Quantize one block with in-block error propagation -> (q, e).
    The reference pads to a power of two (:404-420); padding never feeds a
    real column, so the HIP kernel works on the exact width."""
    for t, nm in ((w_block, "w_block"), (s_block, "s_block"), (z_block, "z_block"),
                  (R_block, "R_block")):
        _lib.require_cuda(t, nm)
    m, B = w_block.shape
    f = lambda t: t.to(torch.float32).contiguous()
    w, s, z, R = f(w_block), f(s_block), f(z_block), f(R_block)
    q = torch.empty_like(w)
    e = torch.empty_like(w)
    with torch.cuda.device(w.device):
        ws = workspace(_lib.lib.tg_process_block_workspace_size(B), w.device)
        call("tg_process_block", stream(), ptr(w), B, ptr(s), B, ptr(z), B, ptr(R), B, m, B,
             int(quantizer.min_q), int(quantizer.max_q), ptr(q), B, ptr(e), B, ptr(ws),
             ws.numel())
    return q, e


# ---------------------------------------------------------------------------
# A8-A12  (gptq_utils.py:459-565)
# ---------------------------------------------------------------------------
def gptq_fwrd(weight_mat: torch.Tensor, H_inv_sqrt: torch.Tensor, quantizer: Quantizer,
              perm: torch.Tensor, block_size: int = 128, use_triton: bool = True,
              R_x: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, int]:
    """Column-wise quantize + error propagation driven by U (= H_inv_sqrt).

    Returns (dequantised W in the original column order and dtype, rank).
    use_triton=True: the TruncGPTQ block kernel semantics (:345-386, :537-545);
    use_triton=False: the GPTQ-comparator column loop (:516-534, :544) --
    round-half-even, error divided by U[c, c], raw U rows for propagation.
    The integer codes of the last call are kept on ``quantizer.codes``
    (uint8, original order, +2^(b-1) offset when sym) for packing.
    A ``Quantizer(weight_format="mxfp4")`` runs the same two procedures on the
    E2M1 grid (tg_gptq_quantize_mx); its codes are the 4-bit E2M1 codes.
    """
    allow_tf32 = torch.backends.cuda.matmul.allow_tf32       # :474-475, restored :565
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        _lib.require_cuda(weight_mat, "gptq_fwrd weight_mat")
        out_features, in_features = weight_mat.shape
        device = weight_mat.device
        orig_dtype = weight_mat.dtype
        weight_mat = weight_mat.to(device=device, dtype=torch.float32).contiguous()
        U = H_inv_sqrt.to(device=device, dtype=torch.float32).contiguous()
        current_rank = U.shape[0]
        if current_rank < in_features:
            logging.info(f"   Rank percent used: {float(current_rank) / in_features:.2%}")
        quantizer.find_params(weight_mat)
        perm_d = perm.to(device=device, dtype=torch.int64).contiguous()
        scale = quantizer.scale.squeeze(-1).contiguous()
        zero = quantizer.zero.squeeze(-1).contiguous()
        Wq = torch.empty_like(weight_mat)
        codes = torch.empty((out_features, in_features), dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            ws = workspace(_lib.lib.tg_quantize_workspace_size(out_features, in_features,
                                                               block_size), device)
            if getattr(quantizer, "weight_format", "int") == "mxfp4":
                call("tg_gptq_quantize_mx", stream(), ptr(weight_mat), out_features, in_features,
                     ptr(U), current_rank, U.shape[1], ptr(perm_d), ptr(scale),
                     _lib.TG_FMT_MXFP4, 0 if use_triton else 1, block_size, ptr(Wq), ptr(codes),
                     ptr(ws), ws.numel())
            else:
                call("tg_gptq_quantize" if use_triton else "tg_gptq_quantize_loop", stream(),
                     ptr(weight_mat), out_features, in_features,
                     ptr(U), current_rank, U.shape[1], ptr(perm_d), ptr(scale), ptr(zero),
                     quantizer.group_size, quantizer.w_bits, int(quantizer.sym), block_size,
                     ptr(Wq), ptr(codes), ptr(ws), ws.numel())
        quantizer.codes = codes
        if R_x is not None:
            log_quantization_error(weight_mat, Wq, R_x, perm_d)
        return Wq.to(dtype=orig_dtype), current_rank
    finally:
        torch.backends.cuda.matmul.allow_tf32 = allow_tf32


# ---------------------------------------------------------------------------
# A13  packing (new; the reference saves dequantised FP16 only, README.md:133)
# ---------------------------------------------------------------------------
def pack_quantized(quantizer: Quantizer, codes: Optional[torch.Tensor] = None):
    """AutoGPTQ-style tensors from the last gptq_fwrd: qweight int32
    (n*b/32, m), qzeros int32 (n/g, m*b/32), scales float32 (n/g, m).
    Static groups in original column order, so no g_idx is needed.
    For ``weight_format="mxfp4"``: (qweight, None, scales) with qweight the same
    4-bit stream of the E2M1 codes and scales the E8M0 bytes, uint8 (n/32, m)."""
    codes = quantizer.codes if codes is None else codes
    m, n = codes.shape
    b = quantizer.w_bits
    if getattr(quantizer, "weight_format", "int") == "mxfp4":
        dev = codes.device
        e8m0 = quantizer.scale_e8m0.contiguous()
        G = e8m0.shape[1]
        qweight = torch.empty((n * 4 // 32, m), dtype=torch.int32, device=dev)
        scales = torch.empty((G, m), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            call("tg_pack_codes", stream(), ptr(codes.contiguous()), m, n, 4, ptr(qweight))
            call("tg_pack_e8m0", stream(), ptr(e8m0), m, G, ptr(scales))
        return qweight, None, scales
    zero = quantizer.zero.squeeze(-1).contiguous()
    G = zero.shape[1]
    dev = codes.device
    qweight = torch.empty((n * b // 32, m), dtype=torch.int32, device=dev)
    qzeros = torch.empty((G, m * b // 32), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("tg_pack_codes", stream(), ptr(codes.contiguous()), m, n, b, ptr(qweight))
        call("tg_pack_zeros", stream(), ptr(zero), m, G, b, int(quantizer.sym), ptr(qzeros))
    scales = quantizer.scale.squeeze(-1).t().contiguous()
    return qweight, qzeros, scales


# ---------------------------------------------------------------------------
# A17  low-rank correction of the residual (new; DESIGN.md "Low-rank correction")
# ---------------------------------------------------------------------------
LOWRANK_MAX = 128


def lowrank_correction(E: torch.Tensor, r: int, *, H: Optional[torch.Tensor] = None,
                       factor: Optional[torch.Tensor] = None,
                       perm: Optional[torch.Tensor] = None, dtype=torch.float32):
    """The rank-r correction A B of the residual E = W - Wq (m x n) that
    minimises tr((E - A B) H (E - A B)^T): (A, B, info), A (m x r) and B
    (r x n) of ``dtype`` (float32, or float64 for checking), balanced per
    direction by a power of two (tg_lrc_factor, include/truncgptq.h).

    H is described by exactly one of
      ``H``       the n x n Hessian itself (float64; the ``gptq`` mode), or
      ``factor``  F (p x n, float64 or float32) with H = F^T F: R_x of
                  process_hessian_alt together with its ``perm``
                  (F[:, perm[j]] = R_x[:, j]), or the scaled sketch Y.
    ``info``: ``mu`` (r float64, the captured eigenvalues of E H E^T, 0 for a
    dropped direction), ``err0`` = tr(E H E^T), ``err1`` = err0 - sum(mu), the
    weighted error that is left, and ``rank``, the number of directions kept
    (those with mu_j > n 2^-52 mu_1).  One host sync."""
    if E.dim() != 2:
        raise ValueError("lowrank_correction: E must be a matrix")
    m, n = E.shape
    r = int(r)
    if not 1 <= r <= LOWRANK_MAX:
        raise ValueError(f"lowrank_correction: r must be in [1, {LOWRANK_MAX}], got {r}")
    if r > min(m, n):
        raise ValueError(f"lowrank_correction: r = {r} exceeds min(m, n) = {min(m, n)}")
    if (H is None) == (factor is None):
        raise ValueError("lowrank_correction: give exactly one of H and factor")
    if H is not None and perm is not None:
        raise ValueError("lowrank_correction: perm goes with factor, not with H")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError("lowrank_correction: dtype must be float32 or float64")
    F = H if factor is None else factor
    if F.dim() != 2 or F.shape[1] != n or (H is not None and F.shape[0] != n):
        raise ValueError(f"lowrank_correction: {'H' if H is not None else 'factor'} has shape "
                         f"{tuple(F.shape)}, E has {n} columns")
    _lib.require_cuda(E, "lowrank_correction E")
    dev = E.device
    Ed = E.to(torch.float32)
    if Ed.stride(1) != 1:
        Ed = Ed.contiguous()
    Fd = F.to(device=dev)
    if H is not None or Fd.dtype != torch.float32:
        Fd = Fd.to(torch.float64)
    if Fd.stride(1) != 1:
        Fd = Fd.contiguous()
    pd = None
    if perm is not None:
        pd = perm.to(device=dev, dtype=torch.int64).contiguous()
        if pd.numel() != n or not torch.equal(torch.sort(pd).values,
                                               torch.arange(n, device=dev)):
            raise ValueError("lowrank_correction: perm must be a permutation of 0 .. n-1")
    gram = int(H is not None)
    p = Fd.shape[0]
    A = torch.empty((m, r), dtype=dtype, device=dev)
    B = torch.empty((r, n), dtype=dtype, device=dev)
    out = torch.empty(r + 1, dtype=torch.float64, device=dev)       # mu, err0
    rank = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws = workspace(_lib.lib.tg_lrc_workspace_size(m, n, p, r, gram), dev)
        call("tg_lrc_factor", stream(), ptr(Ed), m, n, Ed.stride(0), ptr(Fd),
             _lib.DTYPES[Fd.dtype], p, Fd.stride(0), ptr(pd), gram, r, ptr(A), A.stride(0),
             ptr(B), B.stride(0), _lib.DTYPES[dtype], ptr(out), ptr(out[r:]), ptr(rank),
             ptr(ws), ws.numel())
    host = torch.cat((out, rank.to(torch.float64))).cpu().numpy()
    mu, err0 = host[:r].copy(), float(host[r])
    info = dict(mu=mu, err0=err0, err1=err0 - float(mu.sum()), rank=int(host[r + 1]))
    return A, B, info


# ---------------------------------------------------------------------------
# A18  randomised Hadamard rotation (new; DESIGN.md "Hadamard rotation")
# ---------------------------------------------------------------------------
class HadamardRotation:
    """Q = diag(s) (I (x) H_block) / sqrt(block) on `n` input features
    (include/truncgptq.h, A18).  ``x W^T = (x Q)(W Q)^T`` holds exactly and the
    solver's objective is invariant, so a layer is rotated at the two ends of the
    solve: ``rows(W)`` and ``hessian_(H)`` (or ``rows`` on the scaled sketch) go
    in, ``rows(Wq, inverse=True)`` comes back.

    The signs are `sign_bits` (int32, n/32 words, bit j of word i = column
    32 i + j is negated) or are drawn from ``torch.Generator().manual_seed(seed)``
    on the CPU as ``randint(0, 2, (n,))``, so a seed fixes them on every machine;
    exactly one of the two is given.  `block` and `sign_bits` live on `device`."""

    MIN_BLOCK, MAX_BLOCK = 32, 4096

    def __init__(self, n: int, block: int, seed: Optional[int] = None,
                 sign_bits: Optional[torch.Tensor] = None, device="cuda"):
        n, block = int(n), int(block)
        if block < self.MIN_BLOCK or block > self.MAX_BLOCK or block & (block - 1):
            raise ValueError(f"HadamardRotation: block must be a power of two in "
                             f"[{self.MIN_BLOCK}, {self.MAX_BLOCK}], got {block}")
        if n <= 0 or n % block:
            raise ValueError(f"HadamardRotation: block {block} does not divide n = {n}")
        if (seed is None) == (sign_bits is None):
            raise ValueError("HadamardRotation: give exactly one of seed and sign_bits")
        if sign_bits is None:
            neg = torch.randint(0, 2, (n,), generator=torch.Generator().manual_seed(int(seed)))
            words = (neg.reshape(-1, 32) << torch.arange(32, dtype=torch.int64)).sum(dim=1)
            sign_bits = (words - ((words >> 31) << 32)).to(torch.int32)   # two's complement
        elif sign_bits.dtype != torch.int32 or tuple(sign_bits.shape) != (n // 32,):
            raise ValueError(f"HadamardRotation: sign_bits must be int32 of {n // 32} words, got "
                             f"{sign_bits.dtype} {tuple(sign_bits.shape)}")
        self.n, self.block = n, block
        self.sign_bits = sign_bits.detach().to(device).contiguous()

    @classmethod
    def auto_block(cls, n: int) -> int:
        """The largest power of two that divides n, capped at 4096."""
        n = int(n)
        b = min(n & -n, cls.MAX_BLOCK) if n > 0 else 0
        if b < cls.MIN_BLOCK:
            raise ValueError(f"HadamardRotation: n = {n} has no power-of-two factor of at least "
                             f"{cls.MIN_BLOCK}")
        return b

    def rows(self, X: torch.Tensor, inverse: bool = False,
             out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """``X Q`` (``X Q^T`` with `inverse`) on the last dim, a new tensor of
        `out_dtype` (default: X's)."""
        from .qlinear import hadamard
        _lib.require_cuda(X, "HadamardRotation.rows input")
        _lib.require_cuda(self.sign_bits, "HadamardRotation.sign_bits")
        if X.shape[-1] != self.n:
            raise ValueError(f"HadamardRotation.rows: last dim {X.shape[-1]} != n = {self.n}")
        return hadamard(X, self.block, self.sign_bits, inverse=inverse, dtype=out_dtype)

    def hessian_(self, H: torch.Tensor) -> torch.Tensor:
        """``H <- Q^T H Q`` in place (float64, n x n, unit column stride); exactly
        symmetric.  Returns H."""
        _lib.require_cuda(H, "HadamardRotation.hessian_ input")
        _lib.require_cuda(self.sign_bits, "HadamardRotation.sign_bits")
        if H.dim() != 2 or tuple(H.shape) != (self.n, self.n) or H.dtype != torch.float64 \
                or H.stride(1) != 1:
            raise ValueError(f"HadamardRotation.hessian_: H must be float64 ({self.n}, {self.n}) "
                             f"with unit column stride")
        with torch.cuda.device(H.device):
            call("tg_hadamard_sym", stream(), ptr(H), self.n, H.stride(0), self.block,
                 ptr(self.sign_bits))
        return H
