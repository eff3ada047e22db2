#!/usr/bin/env python3
"""Time one packed Mixture-of-Experts layer: QuantExperts (two tg_qgemm_grouped
calls, the sort and the combine) against the only packed alternative there was
before it -- the per-expert loop of the HF experts module with a tg_qgemm /
tg_qgemm_mx call in place of each linear, gathers, nonzero() sync and
index_add_ included -- and against the dense fp16 HF experts forward.

Shape: Qwen3-30B-A3B-like experts, E = 128, H = 2048, I = 768, top-8, at
T in {1, 16, 2048} tokens (--T), int4 g128 and MXFP4.  With R = 8 T slots the
rows regime takes T <= 16; where it does, both regimes are timed
(TG_QGROUPED is read per call).  Beside the whole forward, which up to T = 16
is bound by torch's launches around the two calls, the bare pair of calls is
timed per regime under graph replay (pair_rows, pair_tiles): the crossing of the
regimes is read off those, --T 1 2 4 8 16.

Method (as tools/qgemm_bench.py): the paths alternate inside every run, one
HIP-event bracket each around one forward on each of the weight copies (packed:
3 copies of ~300 MB; dense: 2 copies of 1.2 GB; a 1 GiB buffer is overwritten
before every bracket), per-forward median over --runs brackets.  The whole
measurement is made twice; both medians and their spread are reported.

--act mxfp8 times the MXFP8-activation path instead: the bare pair of
tg_qgemm_grouped_act calls (the activation quantiser inside each) against the
bare pair of tg_qgemm_grouped calls at its production dispatch, MXFP4 experts,
same routing, same method (graph replay over the three weight copies, paths
alternating); act_auto is the production tile height, act_16 / act_64 force one
(TG_QGROUPED_ACT).  Neither the dense module nor the loop is built in this mode.

    python tools/qgrouped_bench.py [--T 1 16 2048] [--act mxfp8] [--out FILE]
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
from gptq_svd_amd.qlinear import QuantExperts, qgemm_grouped  # noqa: E402

DEV = "cuda:0"
E, H, I, K = 128, 2048, 768, 8
BITS, GROUP = 4, 128


def random_experts(gen, fmt):
    """Random words are random codes: every bit pattern is a valid stream."""
    mx = fmt == "mxfp4"
    q = QuantExperts(E, H, I, BITS, GROUP, fmt, device=DEV)
    for name, buf in q.named_buffers():
        if buf.dtype == torch.int32:
            buf.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, buf.shape, generator=gen,
                                    dtype=torch.int64).to(torch.int32))
        elif mx:        # scale bytes 2^-9 .. 2^-6
            buf.copy_(torch.randint(118, 122, buf.shape, generator=gen, dtype=torch.uint8))
        else:
            buf.copy_((torch.rand(buf.shape, generator=gen) * 0.004 + 0.001).half())
    return q


def qgemm(x, q, name, e):
    """x @ W^_e^T of one stack by the single-matrix call."""
    qw, qz, sc = (getattr(q, f"{name}_{k}") for k in ("qweight", "qzeros", "scales"))
    T, (_, _, m), n = x.shape[0], qw.shape, x.shape[1]
    y = torch.empty((T, m), dtype=x.dtype, device=x.device)
    nbytes = L.lib.tg_qgemm_workspace_size(T, m, n)
    ws = L.workspace(nbytes, DEV)
    if qz is None:
        L.call("tg_qgemm_mx", L.stream(), L.ptr(x), L.TG_F16, T, n, L.ptr(qw[e]), L.ptr(sc[e]),
               L.TG_FMT_MXFP4, m, n, None, 0, L.ptr(y), L.TG_F16, m, L.ptr(ws), nbytes)
    else:
        L.call("tg_qgemm", L.stream(), L.ptr(x), L.TG_F16, T, n, L.ptr(qw[e]), L.ptr(qz[e]),
               L.ptr(sc[e]), L.TG_F16, m, n, GROUP, BITS, None, 0, L.ptr(y), L.TG_F16, m, L.ptr(ws),
               nbytes)
    return y


def loop_forward(q, x, idx, w):
    """The HF experts loop with packed linears."""
    out = torch.zeros_like(x)
    mask = torch.nn.functional.one_hot(idx, num_classes=E).permute(2, 1, 0)
    for e in torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero():
        e = int(e[0])
        pos, tok = torch.where(mask[e])
        gu = qgemm(x[tok], q, "gate_up", e)
        h = torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]
        d = qgemm(h, q, "down", e) * w[tok, pos, None]
        out.index_add_(0, tok, d.to(out.dtype))
    return out


def bare_pairs(packs, x, idx, w, regimes, warmup, env="TG_QGROUPED", prefix="pair_",
               act_format=None):
    """{pair_<regime>: (replay, copies)}: the gate_up and down calls alone, on
    routing sorted beforehand, on each weight copy, captured once per regime
    (TG_QGROUPED is read when the call is made, i.e. at capture) and replayed, so
    neither torch's launches around the calls nor the host's launch cost is in
    the bracket.  This is what the `auto` boundary is read from.  With act_format
    the same pair through tg_qgemm_grouped_act, `regimes` being values of `env`."""
    flat = idx.reshape(-1)
    order = torch.argsort(flat, stable=True)
    rows = (order // K).to(torch.int32)
    off = torch.searchsorted(flat[order], torch.arange(E + 1, device=DEV)).to(torch.int32)
    scale = w.reshape(-1)[order].float()
    h = torch.randn(order.numel(), I, device=DEV).half()
    paths = {}
    for regime in regimes:
        os.environ[env] = regime

        def sweep():
            for q in packs:
                qgemm_grouped(x, rows, off, q.gate_up_qweight, q.gate_up_qzeros, q.gate_up_scales,
                              BITS, q.group_size, act_format=act_format)
                qgemm_grouped(h, None, off, q.down_qweight, q.down_qzeros, q.down_scales, BITS,
                              q.group_size, row_scale=scale, act_format=act_format)
        for _ in range(warmup):
            sweep()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            sweep()
        # one replay covers every copy
        paths[prefix + regime] = (lambda i, g=g: g.replay() if i == 0 else None, len(packs))
    return paths


def act_rows(args, gen, flush):
    """--act: one row per T, MXFP4 experts, the two bare pairs side by side."""
    packs = [random_experts(gen, "mxfp4") for _ in range(3)]
    rows = []
    for T in args.T:
        x = torch.randn(T, H, generator=gen).half().to(DEV)
        idx = torch.stack([torch.randperm(E, generator=gen)[:K] for _ in range(T)]).to(DEV)
        w = torch.softmax(torch.randn(T, K, generator=gen), dim=-1).half().to(DEV)
        with torch.no_grad():
            paths = bare_pairs(packs, x, idx, w, ["auto"], args.warmup)
            paths.update(bare_pairs(packs, x, idx, w, ["auto", "16", "64"], args.warmup,
                                    env="TG_QGROUPED_ACT", prefix="act_", act_format=args.act))
            os.environ["TG_QGROUPED_ACT"] = "auto"
            two = [measure(paths, flush, args.warmup, args.runs) for _ in range(2)]
            ref = packs[0](x, idx, w).float()
            packs[0].act_format = args.act
            rel = float((packs[0](x, idx, w).float() - ref).abs().max() / ref.abs().max())
            packs[0].act_format = None
        row = dict(format="mxfp4", act=args.act, T=T, R=T * K, max_rel_diff_vs_16bit=rel)
        for k in paths:
            a, b = two[0][k], two[1][k]
            row[k + "_ms"] = [a, b]
            row[k + "_spread"] = abs(a - b) / min(a, b)
        row["w16_over_act"] = min(two[0]["pair_auto"], two[1]["pair_auto"]) / \
            max(two[0]["act_auto"], two[1]["act_auto"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def measure(paths, flush, warmup, runs):
    """{name: (fn, copies)} -> {name: median ms per forward}; the paths alternate
    inside every run."""
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
    return {k: statistics.median(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qlinear", "qgrouped.json"))
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--T", type=int, nargs="+", default=[1, 16, 2048])
    ap.add_argument("--formats", nargs="+", default=["int", "mxfp4"])
    ap.add_argument("--act", choices=["mxfp8"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qgrouped_bench needs the GPU (there is nothing to time without one)")
    from transformers import Qwen3MoeConfig
    from transformers.models.qwen3_moe.modeling_qwen3_moe import Qwen3MoeExperts
    gen = torch.Generator().manual_seed(0)
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=DEV)
    cfg = Qwen3MoeConfig(hidden_size=H, moe_intermediate_size=I, num_experts=E,
                         num_experts_per_tok=K)
    rows = act_rows(args, gen, flush) if args.act else []
    for fmt in ([] if args.act else args.formats):
        packs = [random_experts(gen, fmt) for _ in range(3)]
        denses = []
        for q in packs[:2]:
            hf = Qwen3MoeExperts(cfg).half().to(DEV)
            hf.gate_up_proj.data, hf.down_proj.data = q.dequantize(torch.float16)
            denses.append(hf)
        for T in args.T:
            x = torch.randn(T, H, generator=gen).half().to(DEV)
            idx = torch.stack([torch.randperm(E, generator=gen)[:K] for _ in range(T)]).to(DEV)
            w = torch.softmax(torch.randn(T, K, generator=gen), dim=-1).half().to(DEV)

            def grouped(regime):
                def fn(i):
                    os.environ["TG_QGROUPED"] = regime
                    packs[i](x, idx, w)
                return fn

            with torch.no_grad():
                paths = {"grouped_auto": (grouped("auto"), 3), "grouped_tiles": (grouped("tiles"), 3),
                         "loop": (lambda i: loop_forward(packs[i], x, idx, w), 3),
                         "dense_fp16": (lambda i: denses[i](x, idx, w), 2)}
                if T * K <= 128:
                    paths["grouped_rows"] = (grouped("rows"), 3)
                paths.update(bare_pairs(packs, x, idx, w, ["rows", "tiles"] if T * K <= 128
                                        else ["tiles"], args.warmup))
                two = [measure(paths, flush, args.warmup, args.runs) for _ in range(2)]
                os.environ["TG_QGROUPED"] = "auto"
                ref = denses[0](x, idx, w).float()
                rel = float((packs[0](x, idx, w).float() - ref).abs().max() / ref.abs().max())
            row = dict(format=fmt, T=T, R=T * K, max_rel_diff_vs_dense=rel)
            for k in paths:
                a, b = two[0][k], two[1][k]
                row[k + "_ms"] = [a, b]
                row[k + "_spread"] = abs(a - b) / min(a, b)
            row["loop_over_grouped"] = min(two[0]["loop"], two[1]["loop"]) / \
                max(two[0]["grouped_auto"], two[1]["grouped_auto"])
            rows.append(row)
            print(json.dumps(row), flush=True)
        del packs, denses
    out = dict(device=torch.cuda.get_device_name(0), E=E, H=H, I=I, top_k=K, bits=BITS, group=GROUP,
               runs=args.runs, warmup=args.warmup,
               method="HIP events around one forward on each weight copy (3 packed, 2 dense), "
                      "per-forward median; 1 GiB overwritten before every bracket; the paths "
                      "alternate inside every run; two whole measurements", rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
