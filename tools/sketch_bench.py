"""Time the fused sketch GEMM (tg_sketch_accum) against the formulation the
facade could otherwise call, the reference's own (gptq_utils.py:196-200):

    Y.addmm_(torch.randn(rank, T, device=...), x.float())

Shapes: n = 4096, fp16 X, T = 16,384 tokens per hook call, rank 4096 and
16,384.  Both variants run in one process, warmed up, timed with device events
over `--reps` rounds in alternating order (fused first in even rounds, torch
first in odd ones); the medians are reported.  TF/s counts 2 rank n T (the
GEMM alone: the fused kernel's Omega generation and the torch variant's randn
and cast are overhead of each, not work).  Peak extra memory is the allocator's
peak above what is live before the call (Y and X).

    python tools/sketch_bench.py [--out profiles/sketch/sketch_accum.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 157.3   # FP32 matrix / vector peak of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--ranks", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sketch", "sketch_accum.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sketch_bench needs a GPU (no fallback)")
    from gptq_svd_amd import _lib
    dev = torch.device("cuda:0")
    n, T = args.n, args.tokens
    x = torch.randn(T, n, generator=torch.Generator().manual_seed(0)).half().to(dev)
    results = []
    for rank in args.ranks:
        Y = torch.zeros((rank, n), dtype=torch.float32, device=dev)

        def fused():
            _lib.call("tg_sketch_accum", _lib.stream(), _lib.ptr(x), _lib.TG_F16, T, n, n, 12345,
                      0, _lib.ptr(Y), rank, n)

        def torch_ref():
            Y.addmm_(torch.randn((rank, T), device=dev, dtype=torch.float32), x.float())

        def timed(fn):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), torch.cuda.max_memory_allocated(dev) - base

        variants = {"fused": fused, "torch": torch_ref}
        for _ in range(args.warmup):
            for fn in variants.values():
                timed(fn)
        ms = {k: [] for k in variants}
        mem = {k: 0 for k in variants}
        for r in range(args.reps):
            order = list(variants) if r % 2 == 0 else list(variants)[::-1]
            for k in order:
                t, m = timed(variants[k])
                ms[k].append(t)
                mem[k] = max(mem[k], m)
        flops = 2.0 * rank * n * T
        row = {"rank": rank, "n": n, "tokens": T, "x_dtype": "fp16", "reps": args.reps}
        for k in variants:
            med = statistics.median(ms[k])
            row[k] = {"ms_median": med, "ms_min": min(ms[k]), "ms_max": max(ms[k]),
                      "tflops": flops / med / 1e9, "of_peak": flops / med / 1e9 / PEAK_TF,
                      "peak_extra_bytes": int(mem[k])}
        row["fused_over_torch_time"] = row["fused"]["ms_median"] / row["torch"]["ms_median"]
        results.append(row)
        print(json.dumps(row), flush=True)
        del Y
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(dev), "peak_tflops_fp32": PEAK_TF,
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
