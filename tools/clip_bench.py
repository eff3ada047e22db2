"""Time the fused clip search (tg_group_params_clip) against a torch
formulation of the same search: a loop over the candidates of elementwise
torch ops on the GPU (scale / zero per candidate, round-to-nearest, the
weighted squared error summed in float64 per group, a running argmin).

Shapes: 4096 x 4096 and 12,288 x 4096, 4-bit asym g128, grid 100 / steps 80
(81 candidates), weighted.  Both variants run in one process, warmed up, timed
with device events over `--reps` rounds in alternating order (fused first in
even rounds, torch first in odd ones); medians with min-max are reported, and
the plain tg_group_params (candidate 0 alone) for scale.  The two variants'
choices are compared once (torch's division and summation order may differ in
the last bit, so near-ties can fall differently).  `share_of_gptq_fwrd` is
the fused median over the solve's 2.54 ms at 4096^2.

    python tools/clip_bench.py [--out profiles/clip/clip_search.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GPTQ_FWRD_MS_4096 = 2.54


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, nargs="+", default=[4096, 4096, 12288, 4096],
                    help="m n pairs")
    ap.add_argument("--bits", type=int, default=4)
    ap.add_argument("--group", type=int, default=128)
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip", "clip_search.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench needs a GPU (no fallback)")
    from gptq_svd_amd import _lib
    dev = torch.device("cuda:0")
    bits, g, grid, steps = args.bits, args.group, args.grid, args.steps
    maxq, minq = float(2 ** bits - 1), 0.0
    results = []
    for m, n in zip(args.shapes[0::2], args.shapes[1::2]):
        G = n // g
        gen = torch.Generator().manual_seed(m + n)
        # Student-t(4) weights, log-normal column weights
        W = (torch.randn(m, n, generator=gen)
             / torch.sqrt(torch.randn(m, n, 4, generator=gen).square().mean(-1)) * 0.02).to(dev)
        h = torch.exp(1.5 * torch.randn(n, generator=gen)).to(dev)
        scale = torch.empty((m, G), dtype=torch.float32, device=dev)
        zero = torch.empty_like(scale)
        choice = torch.empty((m, G), dtype=torch.int32, device=dev)
        objective = torch.empty((m, G, 2), dtype=torch.float64, device=dev)
        kept = {}

        def fused():
            _lib.call("tg_group_params_clip", _lib.stream(), _lib.ptr(W), m, n, n, _lib.ptr(h), g,
                      bits, 0, grid, steps, _lib.ptr(scale), _lib.ptr(zero), _lib.ptr(choice),
                      _lib.ptr(objective))

        def minmax():
            _lib.call("tg_group_params", _lib.stream(), _lib.ptr(W), m, n, n, g, bits, 0,
                      _lib.ptr(scale), _lib.ptr(zero))

        def torch_ref():
            w = W.view(m, G, g)
            hv = h.double().view(1, G, g)
            mn, mx = w.amin(2, keepdim=True), w.amax(2, keepdim=True)
            for i in range(steps + 1):
                p = 1.0 - i / grid
                lo = torch.where(mn < 0, p * mn, mn)
                hi = torch.where(mx > 0, p * mx, mx)
                s = (hi - lo).clamp_min(1e-5) / maxq
                z = torch.round(-lo / s).clamp(0.0, maxq)
                q = torch.round(w / s + z).clamp(minq, maxq)
                e = w - (q - z) * s
                J = (hv * e.double().square()).sum(2, keepdim=True)
                if i == 0:
                    best_j, best_s, best_z = J, s, z
                    best = torch.zeros_like(J, dtype=torch.int32)
                else:
                    better = J < best_j
                    best_j = torch.where(better, J, best_j)
                    best_s = torch.where(better, s, best_s)
                    best_z = torch.where(better, z, best_z)
                    best = torch.where(better, torch.full_like(best, i), best)
            kept["choice"], kept["j"] = best.view(m, G), best_j.view(m, G)

        def timed(fn):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        variants = {"fused": fused, "torch": torch_ref, "minmax": minmax}
        for _ in range(args.warmup):
            for fn in variants.values():
                timed(fn)
        ms = {k: [] for k in variants}
        for r in range(args.reps):
            order = list(variants) if r % 2 == 0 else list(variants)[::-1]
            for k in order:
                ms[k].append(timed(variants[k]))
        fused()
        torch.cuda.synchronize()
        same = float((choice == kept["choice"]).float().mean())
        j_rel = float(((objective[:, :, 1] - kept["j"]).abs()
                       / kept["j"].clamp_min(1e-300)).max())
        row = {"m": m, "n": n, "bits": bits, "sym": False, "group": g, "grid": grid,
               "steps": steps, "candidates": steps + 1, "weighted": True, "reps": args.reps}
        for k in variants:
            row[k] = {"ms_median": statistics.median(ms[k]), "ms_min": min(ms[k]),
                      "ms_max": max(ms[k])}
        row["fused_over_torch_time"] = row["fused"]["ms_median"] / row["torch"]["ms_median"]
        row["torch_over_fused_time"] = row["torch"]["ms_median"] / row["fused"]["ms_median"]
        # element-candidate evaluations per second of the fused kernel
        row["fused_gevals_per_s"] = m * n * (steps + 1) / row["fused"]["ms_median"] / 1e6
        row["choices_equal_to_torch"] = same
        row["chosen_objective_max_rel_diff_to_torch"] = j_rel
        row["groups_moved"] = float((choice != 0).float().mean())
        if (m, n) == (4096, 4096):
            row["share_of_gptq_fwrd"] = row["fused"]["ms_median"] / GPTQ_FWRD_MS_4096
        results.append(row)
        print(json.dumps(row), flush=True)
        del W, scale, zero, choice, objective, kept
        torch.cuda.empty_cache()
    out = {"device": torch.cuda.get_device_name(dev), "gptq_fwrd_ms_4096": GPTQ_FWRD_MS_4096,
           "results": results}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
