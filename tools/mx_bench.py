#!/usr/bin/env python3
"""Time gptq_fwrd on the MXFP4 grid against the integer grid (4-bit, g128) on
the same weight, U and perm -- what the E2M1 step costs in the column chain.

One layer of m x n (default 4096 x 4096): H from seeded random activations,
process_hessian_alt once, then the two quantisers alternate (--runs rounds,
after --warmup rounds), each call between HIP events.  Reported per format:
median and min ms of gptq_fwrd (find_params + the block loop + finalize), and
the relative prediction error of the result; for MXFP4 also that of plain MX
casting (round to nearest, no error feedback) of the same weight.  The integer
format runs twice per round, so the spread of identical work is in the output
("int4_g128" against "int4_g128_again").

    python tools/mx_bench.py [--m 4096 --n 4096] [--out profiles/mx/gptq_fwrd.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gptq_svd_amd.gptq_utils as g  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx", "gptq_fwrd.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx_bench needs the GPU (there is nothing to time without one)")
    gen = torch.Generator().manual_seed(0)
    X = torch.randn(args.tokens, args.n, generator=gen).to(torch.float16).to(DEV)
    X = X * torch.exp(torch.randn(args.n, generator=gen) * 0.5).to(torch.float16).to(DEV)
    W = (torch.randn(args.m, args.n, generator=gen) * 0.05).to(DEV)
    acc = g.HessianAccumulator(args.n, DEV)
    acc.add_batch(X)
    U, R_x, perm = g.process_hessian_alt(acc.get_hessian(), 1e-4, "energy")

    formats = {"int4_g128": dict(w_bits=4, group_size=128),
               "mxfp4": dict(w_bits=4, group_size=32, weight_format="mxfp4"),
               "int4_g128_again": dict(w_bits=4, group_size=128)}
    ms = {k: [] for k in formats}
    out = {}
    for r in range(args.warmup + args.runs):
        for name, kw in formats.items():
            q = g.Quantizer(**kw)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            Wq, k = g.gptq_fwrd(W, U, q, perm, block_size=args.block)
            b.record()
            b.synchronize()
            if r >= args.warmup:
                ms[name].append(a.elapsed_time(b))
            out[name] = Wq
    rows = {}
    for name in formats:
        rows[name] = dict(ms_median=statistics.median(ms[name]), ms_min=min(ms[name]),
                          ms_max=max(ms[name]),
                          pred_error=g.log_quantization_error(W, out[name], R_x, perm))
    # plain MX casting: U = I propagates nothing, so every column is round-to-nearest
    q = g.Quantizer(4, 32, weight_format="mxfp4")
    eye = torch.eye(args.n, device=DEV)
    rtn, _ = g.gptq_fwrd(W, eye, q, torch.arange(args.n, device=DEV), block_size=args.block)
    rows["mxfp4"]["pred_error_plain_casting"] = g.log_quantization_error(W, rtn, R_x, perm)
    res = dict(device=torch.cuda.get_device_name(0), m=args.m, n=args.n, k=int(k),
               block=args.block, runs=args.runs, warmup=args.warmup,
               method="HIP events around gptq_fwrd, formats alternating within a round",
               mx_over_int=rows["mxfp4"]["ms_median"] / rows["int4_g128"]["ms_median"],
               formats=rows)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
