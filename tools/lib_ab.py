"""A/B of library builds (TRUNCGPTQ_LIB) on process_hessian_alt (development
tool): each build runs in its own process on the same seeded H (N = 4096,12288
by default, ROWS x n fp16 rows, default 3n/4), REPS timed solves; prints the
median / min and a hash of (perm, R_x, U) so builds that must be bit-identical
can be compared (and a second one of the spectrum S).  BAND=35,257,...: first
hash (d, e, V2) of tg_band_tridiag on a seeded band of those widths.
    N=12288 python tools/lib_ab.py gptq-svd_amd/variants/lib_band_v*.so"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import hashlib, os, statistics, sys, time, torch
sys.path.insert(0, ROOT)
import gptq_svd_amd.gptq_utils as g
from gptq_svd_amd import _lib
dev = torch.device("cuda")
name = os.path.basename(_lib.LIB_PATH)
for n in [int(x) for x in os.environ.get("BAND", "").split(",") if x]:
    torch.manual_seed(n)
    A = torch.randn(n, n, dtype=torch.float64)
    A = torch.triu(torch.tril(A + A.T, 32), -32).to(dev)
    ws = _lib.workspace(_lib.lib.tg_band_tridiag_workspace_size(n), dev).zero_()
    d, e = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    _lib.call("tg_band_tridiag", _lib.stream(), _lib.ptr(A), n, n, _lib.ptr(d), _lib.ptr(e),
              _lib.ptr(ws), ws.numel())
    torch.cuda.synchronize()
    # V2 (the reflector records) follows the band storage (n x 64 doubles) in the workspace
    off, smax = -(-n * 64 * 8 // 256) * 256, (n - 3) // 32 + 1 if n >= 3 else 1
    h = hashlib.sha1()
    for t in (d, e[:n - 1], ws[off: off + max(1, n - 2) * smax * 32 * 8]):
        h.update(t.contiguous().cpu().numpy().tobytes())
    print(f"{name} band n={n}: hash (d, e, V2) {h.hexdigest()[:16]}", flush=True)
for n in [int(x) for x in os.environ.get("N", "4096,12288").split(",")]:
    rows = int(float(os.environ.get("ROWS", "0.75")) * n)
    torch.manual_seed(1)
    acc = g.HessianAccumulator(n, dev)
    for r0 in range(0, rows, 16384):
        acc.add_batch(torch.randn(min(16384, rows - r0), n, device=dev).half())
    H = acc.get_hessian()
    del acc
    ts = []
    for r in range(int(os.environ.get("REPS", "4")) + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        R, R_x, perm, S, _ = g.truncated_spectral_factor(H, 1e-4, "energy")
        torch.cuda.synchronize()
        if r:
            ts.append(1e3 * (time.perf_counter() - t0))
    h = hashlib.sha1()
    for t in (perm, R_x, R):
        h.update(t.contiguous().cpu().numpy().tobytes())
    hs = hashlib.sha1(S.contiguous().cpu().numpy().tobytes())
    print(f"{name} n={n}: median {statistics.median(ts):.2f} ms, min {min(ts):.2f} ms, "
          f"hash {h.hexdigest()[:16]}, S {hs.hexdigest()[:16]}", flush=True)
'''


def main(libs):
    for lib in libs:
        env = dict(os.environ, TRUNCGPTQ_LIB=os.path.abspath(lib))
        r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], env=env,
                           timeout=600)
        if r.returncode != 0:
            sys.exit(r.returncode)


if __name__ == "__main__":
    main(sys.argv[1:])
