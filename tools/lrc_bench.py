#!/usr/bin/env python3
"""Measurements of the low-rank correction (A17; DESIGN.md "Low-rank correction").

  factor   lowrank_correction (tg_lrc_factor) per layer at 4096 x 4096,
           12288 x 4096 and 4096 x 12288 with r = 32, H given by a full-rank
           factor (p = n, the R_x route), HIP events, median of --runs.
  error    the bench's synthetic 4096^2 layer (X randn fp16 3072 x 4096, W randn):
           the whole solver at 2, 3 and 4 bits (g128) and for mxfp4, then the
           correction of W - Wq at r = 32: err1 / err0 for the f32 factors and
           for their fp16 roundings.
  down     tg_lr_down alone, both regimes, T = 1 .. 512, with the gemv regime's
           split target (TG_LR_TARGET_WGS; 1 = unsplit) and the mfma regime's
           least slabs per split (TG_LR_MIN_SLABS) swept: what decided the
           switch point and the split heuristic.
  forward  the packed forward with and without the correction at T in
           {1, 16, 512}, int4 g128 and mxfp4, the paths alternating inside each
           run as tools/qgemm_bench.py does (weights rotated through >= 768 MB,
           1 GiB overwritten before every bracket, eager launches).

    python tools/lrc_bench.py [--only factor,error,down,forward] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gptq_svd_amd.gptq_utils as G  # noqa: E402
from gptq_svd_amd import _lib as L  # noqa: E402
from qgemm_bench import ROTATE_BYTES, random_packed, timed_alternating  # noqa: E402
import qgemm_bench  # noqa: E402

DEV = "cuda:0"
R = 32


def event_ms(fn, runs, warmup=1):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def bench_factor(args):
    rows = []
    gen = torch.Generator().manual_seed(1)
    for m, n in ((4096, 4096), (12288, 4096), (4096, 12288)):
        E = (torch.randn(m, n, generator=gen) * 0.01).to(DEV)
        F = (torch.randn(n, n, generator=gen, dtype=torch.float64) / n ** 0.5).to(DEV)
        perm = torch.randperm(n, generator=gen).to(DEV)
        med, lo, hi = event_ms(lambda: G.lowrank_correction(E, R, factor=F, perm=perm), args.runs)
        row = dict(m=m, n=n, p=n, r=R, route="m" if m <= n else "p", ms=med, min_ms=lo, max_ms=hi,
                   workspace_GB=L.lib.tg_lrc_workspace_size(m, n, n, R, 0) / 1e9)
        if m == n:
            H = F.t() @ F                                   # setup only
            med, lo, hi = event_ms(lambda: G.lowrank_correction(E, R, H=H), args.runs)
            row.update(gram_ms=med, gram_min_ms=lo, gram_max_ms=hi)
            del H
        rows.append(row)
        print(json.dumps(row), flush=True)
        del E, F
    return rows


def weighted(E, A, B, Rx, perm):
    """tr((E - AB) H (E - AB)^T) with H = Fg^T Fg, in float64 (checking only)."""
    D = (E.double() - A.double() @ B.double())[:, perm]
    return float(((D @ Rx.t()) ** 2).sum())


def bench_error(args):
    rows = []
    gen = torch.Generator().manual_seed(0)
    n = m = 4096
    X = torch.randn(3072, n, generator=gen).half().to(DEV)
    W = torch.randn(m, n, generator=gen).to(DEV)
    acc = G.HessianAccumulator(n, DEV)
    acc.add_batch(X)
    U, R_x, perm = G.process_hessian_alt(acc.get_hessian(), 1e-4, "energy")
    for label, q in (("int2 g128", G.Quantizer(2, 128)), ("int3 g128", G.Quantizer(3, 128)),
                     ("int4 g128", G.Quantizer(4, 128)),
                     ("mxfp4", G.Quantizer(4, 32, weight_format="mxfp4"))):
        Wq, k = G.gptq_fwrd(W, U, q, perm, block_size=1024)
        E = W - Wq
        A, B, info = G.lowrank_correction(E, R, factor=R_x, perm=perm)
        e16 = weighted(E, A.half(), B.half(), R_x, perm)
        row = dict(format=label, rank_k=int(k), r=R, kept=info["rank"], err0=info["err0"],
                   err1=info["err1"], err1_over_err0=info["err1"] / info["err0"],
                   err1_fp16_over_err0=e16 / info["err0"],
                   extra_bits_per_weight=16.0 * R * (m + n) / (m * n))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def down_call(x, B, Z, ws, nbytes):
    T, n = x.shape
    r = B.shape[0]
    L.call("tg_lr_down", L.stream(), L.ptr(x), L.DTYPES[x.dtype], T, n, L.ptr(B),
           L.DTYPES[B.dtype], r, n, n, L.ptr(Z), r, L.ptr(ws), nbytes)


def bench_down(args):
    """Per-call time of tg_lr_down: brackets of 50 eager calls."""
    rows = []
    gen = torch.Generator().manual_seed(2)
    reps = 50
    for n in (4096, 12288):
        B = (torch.randn(R, n, generator=gen) * 0.05).half().to(DEV)
        for T in (1, 2, 4, 8, 16, 32, 64, 512):
            x = torch.randn(T, n, generator=gen).half().to(DEV)
            Z = torch.empty(T, R, dtype=torch.float32, device=DEV)
            row = dict(n=n, r=R, T=T)
            # gemv: the split target (1 = no split: one launch); mfma: the least
            # number of 32-value slabs a split may have
            sweeps = [("gemv", "TG_LR_TARGET_WGS", v) for v in (1, 16, 32, 128, 512, 2048)
                      if T <= 16]
            sweeps += [("mfma", "TG_LR_MIN_SLABS", v) for v in (2, 4, 8, 16, 10 ** 6)]
            for regime, var, val in sweeps:
                os.environ["TG_LR_DOWN"] = regime
                os.environ[var] = str(val)
                nbytes = L.lib.tg_lr_down_workspace_size(T, R, n)
                ws = L.workspace(nbytes, DEV)

                def many():
                    for _ in range(reps):
                        down_call(x, B, Z, ws, nbytes)
                med, lo, hi = event_ms(many, args.runs, warmup=2)
                tag = f"wgs{val}" if regime == "gemv" else f"minslabs{min(val, 9999)}"
                row[f"{regime}_{tag}_us"] = 1e3 * med / reps
                if T > 16:      # below, the workspace is sized for the larger of both regimes
                    row[f"{regime}_{tag}_splits"] = (nbytes - 256) // (4 * T * R) if nbytes else 1
                os.environ.pop(var)
            os.environ.pop("TG_LR_DOWN", None)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def bench_forward(args):
    rows = []
    gen = torch.Generator().manual_seed(3)
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=DEV)
    for fmt in ("int", "mxfp4"):
        qgemm_bench.GROUP = 128 if fmt == "int" else 32
        for m, n in ((4096, 4096), (12288, 4096)):
            first = random_packed(m, n, gen, fmt)
            packed_bytes = sum(t.numel() * t.element_size() for t in first if t is not None)
            lr_bytes = 2 * R * (m + n)
            copies = -(-ROTATE_BYTES // packed_bytes)
            packs = [first] + [tuple(None if t is None else t.clone() for t in first)
                               for _ in range(copies - 1)]
            lrs = [((torch.randn(m, R, generator=gen) * 0.5).half().to(DEV),
                    (torch.randn(R, n, generator=gen) * 0.05).half().to(DEV))
                   for _ in range(copies)]
            for T in (1, 16, 512):
                x = torch.randn(T, n, generator=gen).half().to(DEV)
                y = torch.empty(T, m, dtype=torch.float16, device=DEV)
                y32 = torch.empty(T, m, dtype=torch.float32, device=DEV)
                Z = torch.empty(T, R, dtype=torch.float32, device=DEV)
                nb = L.lib.tg_qgemm_workspace_size(T, m, n)
                ws = L.workspace(nb, DEV)
                nbd = L.lib.tg_lr_down_workspace_size(T, R, n)
                wsd = L.workspace(nbd, DEV)

                def gemm(i, out, out_dt):
                    qw, qz, sc = packs[i]
                    if fmt == "int":
                        L.call("tg_qgemm", L.stream(), L.ptr(x), L.TG_F16, T, n, L.ptr(qw),
                               L.ptr(qz), L.ptr(sc), L.TG_F16, m, n, 128, 4, None, 0, L.ptr(out),
                               out_dt, m, L.ptr(ws), nb)
                    else:
                        L.call("tg_qgemm_mx", L.stream(), L.ptr(x), L.TG_F16, T, n, L.ptr(qw),
                               L.ptr(sc), L.TG_FMT_MXFP4, m, n, None, 0, L.ptr(out), out_dt, m,
                               L.ptr(ws), nb)

                def down(i):
                    down_call(x, lrs[i][1], Z, wsd, nbd)

                def finish(i):
                    A = lrs[i][0]
                    L.call("tg_lr_finish", L.stream(), L.ptr(y32), m, L.ptr(Z), R, L.ptr(A),
                           L.TG_F16, R, T, m, R, None, 0, L.ptr(y), L.TG_F16, m)

                def corrected(i):
                    gemm(i, y32, L.TG_F32)
                    down(i)
                    finish(i)

                paths = {"plain": (lambda i: gemm(i, y, L.TG_F16), copies),
                         "corrected": (corrected, copies),
                         "gemm_f32": (lambda i: gemm(i, y32, L.TG_F32), copies),
                         "down": (down, copies), "finish": (finish, copies)}
                t = timed_alternating(paths, flush, args.warmup, args.runs)
                row = dict(format="int4 g128" if fmt == "int" else "mxfp4", m=m, n=n, T=T, r=R,
                           copies=copies, packed_bytes=packed_bytes, lowrank_bytes=lr_bytes,
                           overhead=t["corrected"][0] / t["plain"][0] - 1.0)
                for k, (med, mn) in t.items():
                    row[k + "_us"], row[k + "_min_us"] = 1e3 * med, 1e3 * mn
                rows.append(row)
                print(json.dumps(row), flush=True)
            del packs, lrs
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="factor,error,down,forward")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lrc", "lrc_bench.json"))
    args = ap.parse_args()
    parts = dict(factor=bench_factor, error=bench_error, down=bench_down, forward=bench_forward)
    out = dict(device=torch.cuda.get_device_name(0), r=R, runs=args.runs, warmup=args.warmup,
               method="HIP events; medians with min (and max); forward: per-call medians over "
                      ">= 768 MB of rotated weight copies, 1 GiB overwritten before every "
                      "bracket, paths alternating inside every run, eager launches; down: "
                      "brackets of 50 eager calls; no perplexity is measured here (no "
                      "weights, no dataset)")
    for name in args.only.split(","):
        out[name] = parts[name](args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
