#!/usr/bin/env python3
"""Measurements of the Hadamard rotation (A18; DESIGN.md "Hadamard rotation").

  kernel   tg_hadamard on fp16 T x n, T in {1, 16, 512, 4096}, n in {4096, 12288},
           block in {128, 1024, 4096}, beside x.clone() of the same tensor (the
           memory-bound yardstick: the same bytes, no arithmetic).  The paths
           alternate inside every run over enough copies of x (and of the output)
           that a sweep moves >= 768 MB or 32 copies, 1 GiB is overwritten before
           every bracket, eager launches, HIP events; bytes = 2 T n in + 2 T n out.
  forward  the packed forward (int4 g128 and mxfp4, 4096 x 4096) with and without
           the rotation at the same T, block 128 and 4096: the modules' own
           forward, weights rotated through >= 768 MB as tools/qgemm_bench.py does.
  error    the solver's weighted error tr((W - Wq) H (W - Wq)^T) with and without
           rotation on the bench's synthetic 4096^2 layer (X randn fp16 3072 x
           4096, W = 0.02 randn) with 16 planted outlier columns (x 30) and the
           same 16 input channels hot (x 10), for int4 g128, int3 g128 and mxfp4,
           automatic block (4096).

    python tools/had_bench.py [--only kernel,forward,error] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gptq_svd_amd.gptq_utils as G  # noqa: E402
from gptq_svd_amd import _lib as L  # noqa: E402
from gptq_svd_amd.qlinear import MXQuantLinear, QuantLinear  # noqa: E402
from qgemm_bench import ROTATE_BYTES, random_packed, timed_alternating  # noqa: E402
import qgemm_bench  # noqa: E402

DEV = "cuda:0"
TS = (1, 16, 512, 4096)


def bench_kernel(args):
    rows = []
    gen = torch.Generator().manual_seed(0)
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=DEV)
    for n in (4096, 12288):
        for T in TS:
            nbytes = 4 * T * n                                   # in + out, fp16
            copies = max(1, min(32, -(-ROTATE_BYTES // nbytes)))
            xs = [torch.randn(T, n, generator=gen).half().to(DEV) for _ in range(copies)]
            ys = [torch.empty_like(x) for x in xs]
            for b in (128, 1024, 4096):
                rot = G.HadamardRotation(n, b, seed=1, device=DEV)
                sign = rot.sign_bits

                def had(i):
                    L.call("tg_hadamard", L.stream(), L.ptr(xs[i]), L.TG_F16, T, n, n, b,
                           L.ptr(sign), 0, L.ptr(ys[i]), L.TG_F16, n)

                def copy(i):
                    ys[i].copy_(xs[i])

                def clone(i):
                    xs[i].clone()

                t = timed_alternating({"hadamard": (had, copies), "copy": (copy, copies),
                                       "clone": (clone, copies)}, flush, args.warmup, args.runs)
                row = dict(T=T, n=n, block=b, copies=copies, bytes=nbytes,
                           ratio_to_clone=t["hadamard"][0] / t["clone"][0],
                           ratio_to_copy=t["hadamard"][0] / t["copy"][0],
                           hadamard_GBps=nbytes / (1e6 * t["hadamard"][0]),
                           clone_GBps=nbytes / (1e6 * t["clone"][0]))
                for k, (med, mn) in t.items():
                    row[k + "_us"], row[k + "_min_us"] = 1e3 * med, 1e3 * mn
                rows.append(row)
                print(json.dumps(row), flush=True)
            del xs, ys
    return rows


def bench_forward(args):
    rows = []
    gen = torch.Generator().manual_seed(3)
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=DEV)
    m = n = 4096
    for fmt in ("int", "mxfp4"):
        qgemm_bench.GROUP = 128 if fmt == "int" else 32
        first = random_packed(m, n, gen, fmt)
        packed_bytes = sum(t.numel() * t.element_size() for t in first if t is not None)
        copies = -(-ROTATE_BYTES // packed_bytes)
        for b in (128, 4096):
            sign = G.HadamardRotation(n, b, seed=2, device=DEV).sign_bits

            def module(rotation):
                qw, qz, sc = first
                if fmt == "int":
                    return QuantLinear.from_packed(qw, qz, sc, 4, 128, rotation=rotation)
                return MXQuantLinear.from_packed(qw, sc, rotation=rotation)

            plain = [module(None) for _ in range(copies)]
            rotated = [module((b, sign)) for _ in range(copies)]
            for T in TS:
                x = torch.randn(T, n, generator=gen).half().to(DEV)
                t = timed_alternating({"plain": (lambda i: plain[i](x), copies),
                                       "rotated": (lambda i: rotated[i](x), copies)},
                                      flush, args.warmup, args.runs)
                row = dict(format="int4 g128" if fmt == "int" else "mxfp4", m=m, n=n, T=T,
                           block=b, copies=copies,
                           overhead=t["rotated"][0] / t["plain"][0] - 1.0)
                for k, (med, mn) in t.items():
                    row[k + "_us"], row[k + "_min_us"] = 1e3 * med, 1e3 * mn
                rows.append(row)
                print(json.dumps(row), flush=True)
            del plain, rotated
    return rows


def weighted(W, Wq, H):
    D = (W.double() - Wq.double())
    return float(((D @ H) * D).sum())


def bench_error(args):
    rows = []
    gen = torch.Generator().manual_seed(0)
    n = m = 4096
    hot = torch.randperm(n, generator=gen)[:16]
    X = torch.randn(3072, n, generator=gen)
    X[:, hot] *= 10.0
    W = 0.02 * torch.randn(m, n, generator=gen)
    W[:, hot] *= 30.0
    X, W = X.half().to(DEV), W.to(DEV)
    acc = G.HessianAccumulator(n, DEV)
    acc.add_batch(X)
    H = acc.get_hessian()
    rot = G.HadamardRotation(n, G.HadamardRotation.auto_block(n), seed=0, device=DEV)
    Hr = rot.hessian_(H.clone())
    Wr = rot.rows(W)
    sides = {}
    for tag, (Wx, Hx) in (("plain", (W, H)), ("rotated", (Wr, Hr))):
        U, R_x, perm = G.process_hessian_alt(Hx.clone(), 1e-4, "energy")
        sides[tag] = (Wx, Hx, U, perm)
    for label, mk in (("int4 g128", lambda: G.Quantizer(4, 128)),
                      ("int3 g128", lambda: G.Quantizer(3, 128)),
                      ("mxfp4", lambda: G.Quantizer(4, 32, weight_format="mxfp4"))):
        row = dict(format=label, block=rot.block)
        for tag, (Wx, Hx, U, perm) in sides.items():
            Wq, k = G.gptq_fwrd(Wx, U, mk(), perm, block_size=1024)
            row[f"{tag}_err"], row[f"{tag}_rank_k"] = weighted(Wx, Wq, Hx), int(k)
        row["plain_over_rotated"] = row["plain_err"] / row["rotated_err"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="kernel,forward,error")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "had", "had_bench.json"))
    args = ap.parse_args()
    parts = dict(kernel=bench_kernel, forward=bench_forward, error=bench_error)
    out = dict(device=torch.cuda.get_device_name(0), runs=args.runs, warmup=args.warmup,
               method="HIP events; per-call medians with min; paths alternating inside every "
                      "run over rotated copies (>= 768 MB or 32 copies), 1 GiB overwritten "
                      "before every bracket, eager launches; no perplexity is measured here "
                      "(no weights, no dataset)")
    for name in args.only.split(","):
        out[name] = parts[name](args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
