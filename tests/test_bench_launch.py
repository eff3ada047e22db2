"""bench.py's --gpus contract on the CPU (no GPU needed): a launcher's
WORLD_SIZE must equal --gpus, and --gpus N > 1 without a launcher spawns N
ranks instead of silently running one.  Also --dump-outputs' file format and
the --full switch."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_launch_plan():
    assert bench.launch_plan(1, {}) == ("run", 1)
    assert bench.launch_plan(4, {}) == ("spawn", 4)
    assert bench.launch_plan(2, {"WORLD_SIZE": "2"}) == ("run", 2)
    with pytest.raises(SystemExit, match="must agree"):
        bench.launch_plan(2, {"WORLD_SIZE": "3"})
    with pytest.raises(SystemExit):
        bench.launch_plan(0, {})


def test_mismatched_world_fails_loudly():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "must agree" in r.stderr


def test_dump_outputs_fixed_sample(tmp_path):
    """--dump-outputs: float32 stays float32, everything else becomes float64
    (exact for the packed int32 words), a large output is written as the same
    seeded sample of DUMP_SAMPLE values on every call, and eight outputs of
    any size stay under 64 MB."""
    import numpy as np
    import torch
    big = bench.DUMP_SAMPLE + 12345
    big -= big % 5
    outs = dict(R=torch.arange(big, dtype=torch.float64) * 0.5,
                Wq=torch.arange(big, dtype=torch.float32).reshape(-1, 5),
                qweight=torch.tensor([[-2 ** 31, 2 ** 31 - 1], [7, -1]], dtype=torch.int32),
                perm=torch.tensor([2, 0, 1]), k=torch.tensor(3))
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), outs)
    bench.dump_outputs(str(b), outs)
    got = {n: np.load(a / f"{n}.npy") for n in outs}
    for n in outs:
        assert np.array_equal(got[n], np.load(b / f"{n}.npy")), n
    assert got["Wq"].dtype == np.float32
    assert all(got[n].dtype == np.float64 for n in ("R", "qweight", "perm", "k"))
    assert got["qweight"].tolist() == [-2.0 ** 31, 2.0 ** 31 - 1, 7.0, -1.0]
    assert got["perm"].tolist() == [2.0, 0.0, 1.0] and got["k"].tolist() == [3.0]
    # the sample: DUMP_SAMPLE values of the flattened output at sorted indices
    # (R[i] = i / 2, Wq.flatten()[i] = i), the same indices for the same size
    assert got["R"].shape == got["Wq"].shape == (bench.DUMP_SAMPLE,)
    idx = got["R"] * 2
    assert np.all(np.diff(idx) >= 0) and idx[-1] < big and len(np.unique(idx)) > big // 2
    assert np.array_equal(idx, got["Wq"].astype(np.float64))
    assert (6 * 8 + 2 * 4) * bench.DUMP_SAMPLE <= 64 * 10 ** 6  # six float64, two float32


def test_full_and_dump_options_are_off_by_default():
    """The extras (phases, large widths, end-to-end shapes, CPU baseline) run
    only with --full, the dump only with --dump-outputs."""
    old = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1"]
        args = bench.parse()
        assert not args.full and args.dump_outputs is None and (args.steps, args.warmup) == (2, 1)
        sys.argv += ["--full", "--dump-outputs", "d"]
        args = bench.parse()
        assert args.full and args.dump_outputs == "d"
    finally:
        sys.argv = old
