"""CPU: the harness's clip-search switch through the multi-GPU plumbing
(gloo, world_size 2), with test_dist_harness.py's CPU stand-ins for the HIP
solver calls.  The stand-in gptq_fwrd takes scale / zero from the numpy
restatement of the search (tests/clip_ref.py) whenever the Quantizer it is
handed asks for it, so this checks what the harness is responsible for: every
module's Quantizer carries the settings and diag(H) of its group's Hessian,
rows quantised by their owners are bit-identical to the one-process run, and
the per-group search results are gathered into the same layer_stats.
"""
import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import clip_ref
from test_dist_harness import PATCHED, _free_port, _patch, tiny_model

GRID, STEPS = 20, 12


@pytest.fixture(autouse=True)
def restore_harness(monkeypatch):
    import gptq_svd_amd.harness as harness
    for name in PATCHED:
        monkeypatch.setattr(harness, name, getattr(harness, name))


def _patch_clip(harness, hs, seen):
    """_patch, with a gptq_fwrd stand-in that honours Quantizer.clip_search."""
    from oracle import oracle as o
    _patch(harness, hs)
    plain = harness.gptq_fwrd

    def fwrd(W, R, q, perm, block_size=1024, use_triton=True, R_x=None):
        if not q.clip_search:
            return plain(W, R, q, perm, block_size, use_triton, R_x)
        Wn = W.float().numpy()
        h = q.col_weight.float().clamp_min(0).numpy()
        seen.append((q.clip_grid, q.clip_steps, h.copy()))
        ref = clip_ref.clip_search(Wn, h, q.w_bits, q.group_size, q.sym, q.clip_grid, q.clip_steps)
        idx = ref["choice"][:, :, None].astype(np.int64)
        at = lambda a: np.take_along_axis(a, idx, axis=2)[:, :, 0].copy()
        real = o.find_params
        o.find_params = lambda *a: (at(ref["s"]), at(ref["z"]))
        try:
            Wq, k = plain(W, R, q, perm, block_size, use_triton, R_x)
        finally:
            o.find_params = real
        q.clip_choice = torch.from_numpy(ref["choice"].copy())
        q.clip_objective = torch.from_numpy(np.stack([ref["J"][:, :, 0], at(ref["J"])], axis=2))
        return Wq, k

    harness.gptq_fwrd = fwrd


def _run(ids, **kw):
    import gptq_svd_amd.harness as harness
    hs, seen = [], []
    _patch_clip(harness, hs, seen)
    model = tiny_model("opt", 5)
    res = harness.quantize_model(model, ids, mode="eigh", w_bits=3, group_size=64, sym=True,
                                 eps=1e-3, threshold_method="energy", batch_size=2, device="cpu",
                                 **kw)
    W = {n: p.detach().clone().numpy() for n, p in model.named_parameters()
         if n.endswith("weight") and "layers" in n and p.dim() == 2}
    return hs, seen, res, W


def _worker(rank, world, port, ids, out):
    import os
    torch.set_num_threads(1)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _, _, res, W = _run(ids, clip_search=True, clip_grid=GRID, clip_steps=STEPS)
        out[rank] = dict(W=W, stats=[{k: v for k, v in s.items() if k != "time"}
                                     for s in res["layer_stats"]])
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_clip_search_through_the_harness_and_row_sharding():
    torch.set_num_threads(2)
    gen = torch.Generator().manual_seed(9)
    ids = [torch.randint(0, 256, (1, 16), generator=gen) for _ in range(6)]
    hs, seen, res, W = _run(ids, clip_search=True, clip_grid=GRID, clip_steps=STEPS)
    _, seen_off, res_off, W_off = _run(ids)

    # every module's Quantizer got the settings and its group's diag(H)
    groups = [3, 1, 1, 1] * 2                       # q/k/v, out_proj, fc1, fc2 per layer
    assert len(hs) == 8 and len(seen) == sum(groups) == len(res["layer_stats"])
    it = iter(seen)
    for H, cnt in zip(hs, groups):
        for _ in range(cnt):
            grid, steps, h = next(it)
            assert (grid, steps) == (GRID, STEPS)
            assert np.array_equal(h, torch.diagonal(H).float().numpy())
    for s in res["layer_stats"]:
        assert s["clip_j"] <= s["clip_j0"] and 0 <= s["clip_moved"] <= s["clip_groups"]
    assert sum(s["clip_moved"] for s in res["layer_stats"]) > 0
    assert any(not np.array_equal(W[k], W_off[k]) for k in W)
    assert not seen_off and all("clip_j" not in s for s in res_off["layer_stats"])

    manager = mp.Manager()
    out = manager.dict()
    mp.spawn(_worker, args=(2, _free_port(), ids, out), nprocs=2, join=True)
    r0, r1 = out[0], out[1]
    assert W.keys() == r0["W"].keys() == r1["W"].keys()
    for name in W:
        assert np.array_equal(r0["W"][name], r1["W"][name]), name
    # the ranks' all-reduced H differs from the one-process H in the last bits
    # (order of the FP64 additions), which can flip a code at a rounding tie;
    # the search results of rows owned by different ranks must still add up to
    # the same per-module record on both ranks
    assert r0["stats"] == r1["stats"]
    assert [s["clip_groups"] for s in r0["stats"]] == [s["clip_groups"]
                                                       for s in res["layer_stats"]]
    same = sum(np.array_equal(r0["W"][n], W[n]) for n in W)
    print(f"{same} of {len(W)} weights bit-identical to the one-process run")
    assert same == len(W)
