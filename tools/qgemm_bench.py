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

--format mxfp4 --act mxfp8 times the block-scaled W4A8 path tg_qgemm_mx_act
beside the weights-only tg_qgemm_mx, the dense fp16 matmul and the activation
quantiser alone, alternating inside every run (eager launches); --other-lib
adds tg_qgemm_mx and tg_qgemm of another build of the library, alternating too.

    python tools/qgemm_bench.py [--graph] [--format int|mxfp4] [--group G] [--out FILE]
    python tools/qgemm_bench.py --format mxfp4 --act mxfp8 [--other-lib SO] [--out FILE]
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


def timed_alternating(paths, flush, warmup, runs):
    """{name: (fn, copies)} -> {name: (median ms, min ms)} per call.  Every run
    times each path once, one after the other, so that drift of the device's
    clocks falls on all of them alike."""
    for fn, copies in paths.values():
        for _ in range(warmup):
            for i in range(copies):
                fn(i)
    ms = {k: [] for k in paths}
    for _ in range(runs):
        for name, (fn, copies) in paths.items():
            flush.zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(copies):
                fn(i)
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / copies)
    return {k: (statistics.median(v), min(v)) for k, v in ms.items()}


def bind_other(path):
    """A second build of the library (e.g. the parent commit's) for A/B timing."""
    import ctypes
    other = ctypes.CDLL(path)
    for name in ("tg_qgemm", "tg_qgemm_mx"):
        fn = getattr(other, name)
        fn.argtypes, fn.restype = L._SIGS[name]
    return other


def main_act(args):
    """--format mxfp4 --act mxfp8: tg_qgemm_mx_act beside the weights-only
    tg_qgemm_mx, the dense fp16 matmul and the quantiser alone, alternating in
    one process; with --other-lib also tg_qgemm_mx and tg_qgemm (int4, g128) of
    this build against the other build's."""
    global GROUP
    gen = torch.Generator().manual_seed(0)
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=DEV)
    other = bind_other(args.other_lib) if args.other_lib else None
    rows = []
    for m, n in ((4096, 4096), (12288, 4096)):
        GROUP = 32
        qw, _, sc = random_packed(m, n, gen, "mxfp4")
        dense = dequantize_packed_mx(qw, sc, torch.float16)
        packed_bytes = qw.numel() * 4 + sc.numel()
        pc = -(-ROTATE_BYTES // packed_bytes)
        dc = -(-ROTATE_BYTES // (dense.numel() * 2))
        packs = [(qw, sc)] + [(qw.clone(), sc.clone()) for _ in range(pc - 1)]
        denses = [dense] + [dense.clone() for _ in range(dc - 1)]
        if other is not None:
            GROUP = 128
            ipacks = [random_packed(m, n, gen, "int") for _ in range(pc)]
        for T in args.T:
            x = torch.randn(T, n, generator=gen).to(torch.float16).to(DEV)
            y = torch.empty(T, m, dtype=torch.float16, device=DEV)
            xq = torch.empty(T, n, dtype=torch.uint8, device=DEV)
            xs = torch.empty(T, n // 32, dtype=torch.uint8, device=DEV)
            nb_w = L.lib.tg_qgemm_workspace_size(T, m, n)
            nb_a = L.lib.tg_qgemm_mx_act_workspace_size(T, m, n)
            ws_w, ws_a = L.workspace(nb_w, DEV), L.workspace(nb_a, DEV)

            def act_call(i):
                a, c = packs[i]
                L.call("tg_qgemm_mx_act", L.stream(), L.ptr(x), L.TG_F16, T, n, L.ptr(a), L.ptr(c),
                       L.TG_FMT_MXFP4, L.TG_ACT_MXFP8, m, n, None, 0, L.ptr(y), L.TG_F16, m,
                       L.ptr(ws_a), nb_a)

            def mx_args(i):
                a, c = packs[i]
                return (L.stream(), L.ptr(x), L.TG_F16, T, n, L.ptr(a), L.ptr(c), L.TG_FMT_MXFP4, m,
                        n, None, 0, L.ptr(y), L.TG_F16, m, L.ptr(ws_w), nb_w)

            def int_args(i):
                a, b, c = ipacks[i]
                return (L.stream(), L.ptr(x), L.TG_F16, T, n, L.ptr(a), L.ptr(b), L.ptr(c), L.TG_F16,
                        m, n, 128, BITS, None, 0, L.ptr(y), L.TG_F16, m, L.ptr(ws_w), nb_w)

            def quant_call(i):
                L.call("tg_quant_act_mx", L.stream(), L.ptr(x), L.TG_F16, T, n, n, L.TG_ACT_MXFP8,
                       L.ptr(xq), n, L.ptr(xs))

            paths = {"act": (act_call, pc),
                     "weights_only": (lambda i: L.call("tg_qgemm_mx", *mx_args(i)), pc),
                     "dense": (lambda i: torch.nn.functional.linear(x, denses[i]), dc),
                     "quant": (quant_call, pc)}
            if other is not None:
                paths["weights_only_other"] = (lambda i: other.tg_qgemm_mx(*mx_args(i)), pc)
                paths["int4"] = (lambda i: L.call("tg_qgemm", *int_args(i)), pc)
                paths["int4_other"] = (lambda i: other.tg_qgemm(*int_args(i)), pc)
            t = timed_alternating(paths, flush, args.warmup, args.runs)
            act_call(0)
            ref = torch.nn.functional.linear(x, dense).float()
            rel = float((y.float() - ref).norm() / ref.norm())
            row = dict(m=m, n=n, T=T, packed_copies=pc, dense_copies=dc,
                       rel_diff_vs_dense=rel,
                       act_TFLOPs=2.0 * T * m * n / (t["act"][0] * 1e-3) / 1e12,
                       act_GBps=packed_bytes / (t["act"][0] * 1e-3) / 1e9)
            for k, (med, mn) in t.items():
                row[k + "_ms"], row[k + "_min_ms"] = med, mn
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), format="mxfp4", act="mxfp8", dtype="float16",
               runs=args.runs, warmup=args.warmup, launch="eager",
               method="HIP events around one call on each of >= 768 MB of weight copies, "
                      "per-call median; 1 GiB overwritten before every bracket; the paths "
                      "alternate inside every run", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


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
    ap.add_argument("--act", choices=["mxfp8"], default=None,
                    help="with --format mxfp4: time tg_qgemm_mx_act beside the other paths")
    ap.add_argument("--other-lib", default=None,
                    help="with --act: another build of libtruncgptq.so to time against")
    args = ap.parse_args()
    mx = args.format == "mxfp4"
    GROUP = 32 if mx else args.group
    if args.act and not mx:
        raise SystemExit("--act needs --format mxfp4")
    if not torch.cuda.is_available():
        raise SystemExit("qgemm_bench needs the GPU (there is nothing to time without one)")
    if args.act:
        return main_act(args)
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
