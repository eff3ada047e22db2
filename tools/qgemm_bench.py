#!/usr/bin/env python3
"""Time tg_qgemm (4-bit, g128, fp16) against torch.nn.functional.linear on the
dense fp16 dequantised weight -- what a user has without the packed path.

Shapes: m = n = 4096 and (m, n) = (12288, 4096) (Qwen3-8B hidden and MLP-up
widths), T in {1, 8, 64, 512}.  A run is one HIP-event bracket around one call
on each of COPIES distinct copies of the weight (together 768 MB or more,
three times the 256 MB last-level cache, and a 1 GiB buffer is overwritten
before every run), so every call re-reads its weight from HBM and the
bracket is long enough to time; the time of a call is the bracket over COPIES.
Reported: the median of --runs runs after --warmup warm-up runs, and for the
packed path the achieved GB/s of packed bytes (qweight + qzeros + scales).

--format mxfp4 times tg_qgemm_mx on an MXFP4 image instead (E2M1 codes, one
E8M0 byte per 32 values: the same bytes per weight as int4 at --group 32, the
comparison that isolates the decode); --group sets the integer group size.

--graph replays a captured graph of the same calls, so that the host's launch
cost (which bounds the eager T = 1 numbers) is not in the bracket.

    python tools/qgemm_bench.py [--graph] [--format int|mxfp4] [--group G] [--out FILE]
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

from gptq_svd_amd import _lib as L  # noqa: E402
from gptq_svd_amd.qlinear import dequantize_packed, dequantize_packed_mx  # noqa: E402

DEV = "cuda:0"
BITS, GROUP = 4, 128


def random_packed(m, n, gen, fmt="int"):
    """Random words are random codes: every bit pattern is a valid stream.
    mxfp4: (qweight, None, scale bytes 110 .. 125, i.e. scales 2^-17 .. 2^-2)."""
    qw = torch.randint(-2 ** 31, 2 ** 31 - 1, (n * BITS // 32, m), generator=gen,
                       dtype=torch.int64).to(torch.int32).to(DEV)
    if fmt == "mxfp4":
        return qw, None, torch.randint(110, 126, (n // 32, m), generator=gen,
                                       dtype=torch.uint8).to(DEV)
    qz = torch.randint(-2 ** 31, 2 ** 31 - 1, (n // GROUP, m * BITS // 32), generator=gen,
                       dtype=torch.int64).to(torch.int32).to(DEV)
    sc = (torch.rand(n // GROUP, m, generator=gen) * 0.01 + 0.002).to(torch.float16).to(DEV)
    return qw, qz, sc


ROTATE_BYTES = 768 << 20


def timed(fn, copies, flush, warmup, runs, graph=False):
    """Per-call ms (median, min) of fn(i), i over the weight copies.  graph:
    the sweep over the copies is captured once and replayed, which takes the
    host's launch cost out of the bracket."""
    def sweep():
        for i in range(copies):
            fn(i)
    for _ in range(warmup):
        sweep()
    if graph:
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            sweep()
        sweep = g.replay
        sweep()
    ms = []
    for _ in range(runs):
        flush.zero_()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        sweep()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / copies)
    return statistics.median(ms), min(ms)


def main():
    global GROUP
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qlinear", "qgemm.json"))
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--T", type=int, nargs="+", default=[1, 8, 64, 512])
    ap.add_argument("--graph", action="store_true",
                    help="time a captured graph of the calls instead of eager launches")
    ap.add_argument("--format", choices=["int", "mxfp4"], default="int")
    ap.add_argument("--group", type=int, default=GROUP, help="integer group size (format int)")
    args = ap.parse_args()
    mx = args.format == "mxfp4"
    GROUP = 32 if mx else args.group
    if not torch.cuda.is_available():
        raise SystemExit("qgemm_bench needs the GPU (there is nothing to time without one)")
    gen = torch.Generator().manual_seed(0)
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=DEV)
    forced = os.environ.get("TG_QGEMM") if os.environ.get("TG_QGEMM") in ("gemv", "mfma") else None
    rows = []
    for m, n in ((4096, 4096), (12288, 4096)):
        qw, qz, sc = random_packed(m, n, gen, args.format)
        if mx:
            dense = dequantize_packed_mx(qw, sc, torch.float16)
            packed_bytes = qw.numel() * 4 + sc.numel()
        else:
            dense = dequantize_packed(qw, qz, sc, BITS, GROUP, torch.float16)
            packed_bytes = qw.numel() * 4 + qz.numel() * 4 + sc.numel() * 2
        pc = -(-ROTATE_BYTES // packed_bytes)
        dc = -(-ROTATE_BYTES // (dense.numel() * 2))
        packs = [(qw, qz, sc)] + [(qw.clone(), None if mx else qz.clone(), sc.clone())
                                  for _ in range(pc - 1)]
        denses = [dense] + [dense.clone() for _ in range(dc - 1)]
        for T in args.T:
            x = torch.randn(T, n, generator=gen).to(torch.float16).to(DEV)
            y = torch.empty(T, m, dtype=torch.float16, device=DEV)
            nbytes = L.lib.tg_qgemm_workspace_size(T, m, n)
            ws = L.workspace(nbytes, DEV)

            def packed_call(i):
                a, b, c = packs[i]
                if mx:
                    L.call("tg_qgemm_mx", L.stream(), L.ptr(x), L.TG_F16, T, n, L.ptr(a), L.ptr(c),
                           L.TG_FMT_MXFP4, m, n, None, 0, L.ptr(y), L.TG_F16, m, L.ptr(ws), nbytes)
                    return
                L.call("tg_qgemm", L.stream(), L.ptr(x), L.TG_F16, T, n, L.ptr(a), L.ptr(b),
                       L.ptr(c), L.TG_F16, m, n, GROUP, BITS, None, 0, L.ptr(y), L.TG_F16, m,
                       L.ptr(ws), nbytes)

            def dense_call(i):
                torch.nn.functional.linear(x, denses[i])

            p_med, p_min = timed(packed_call, pc, flush, args.warmup, args.runs, args.graph)
            d_med, d_min = timed(dense_call, dc, flush, args.warmup, args.runs, args.graph)
            packed_call(0)
            ref = torch.nn.functional.linear(x, dense).float()
            rel = float((y.float() - ref).abs().max() / ref.abs().max())
            row = dict(m=m, n=n, T=T, regime=forced or ("gemv" if T <= 4 else "mfma"),
                       packed_copies=pc, dense_copies=dc, packed_ms=p_med, packed_min_ms=p_min, dense_ms=d_med, dense_min_ms=d_min,
                       speedup=d_med / p_med, packed_GBps=packed_bytes / (p_med * 1e-3) / 1e9,
                       dense_GBps=dense.numel() * 2 / (d_med * 1e-3) / 1e9,
                       packed_TFLOPs=2.0 * T * m * n / (p_med * 1e-3) / 1e12,
                       max_rel_diff_vs_dense=rel)
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), format=args.format, bits=BITS, group=GROUP,
               dtype="float16",
               runs=args.runs, warmup=args.warmup, launch="graph" if args.graph else "eager",
               method="HIP events around one call on each of >= 768 MB of weight copies, "
                      "per-call median; 1 GiB overwritten before every run",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
