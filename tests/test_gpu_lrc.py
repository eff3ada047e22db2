"""GPU: tg_lrc_factor / gptq_utils.lowrank_correction against the float64
restatement of tests/lrc_ref.py (which tests/test_lrc_ref.py proves on the CPU
to 1e-10, a 100x margin under the bars here).

A and B are never compared alone (the sign of a direction is free): the bars are
on A B (1e-8 ||E||_F), mu (1e-10 mu_1), err1 against the directly evaluated
tr((E - AB) H (E - AB)^T) (1e-8 relative) and A0^T A0 = I (1e-8).  They are
taken on the library's float64 outputs; the float32 outputs, which are what the
harness stores, must be the one rounding of those, bit for bit (a float32 A B
alone differs from the float64 one by ~5e-8 ||AB||, the rounding of its factors).
"""
import ctypes

import numpy as np
import pytest
import torch

import lrc_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g():
    import gptq_svd_amd.gptq_utils as g
    return g


@pytest.fixture(scope="module")
def lib():
    from gptq_svd_amd import _lib
    return _lib


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def fro(a):
    return float(np.linalg.norm(a))


def bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


def h_args(c):
    """The keyword arguments that describe H to lowrank_correction."""
    if c["kind"] == "gram":
        return dict(H=dev(c["H"]))
    if c["kind"] == "sketch":
        return dict(factor=dev(c["F"]))
    return dict(factor=dev(c["F"][:, c["perm"]]), perm=dev(c["perm"]))   # Rx[:, j] = F[:, perm[j]]


def solve(g, c, dtype=torch.float64):
    A, B, info = g.lowrank_correction(dev(c["E"]), c["r"], dtype=dtype, **h_args(c))
    return A.cpu().numpy(), B.cpu().numpy(), info


def check_against_reference(tag, c, A, B, info, rank=None):
    E = c["E"].astype(np.float64)
    r = c["r"]
    A0r, B0r, ref = L.reference(c)
    rank = r if rank is None else rank
    assert np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(info["mu"]).all()
    AB = A @ B
    e_ab = fro(AB - A0r @ B0r) / fro(E)
    e_mu = float(np.max(np.abs(info["mu"] - ref["mu"]))) / ref["mu"][0]
    e_e0 = abs(info["err0"] - ref["err0"]) / ref["err0"]
    A0 = L.unbalance(A)
    e_orth = float(np.max(np.abs(A0[:, :rank].T @ A0[:, :rank] - np.eye(rank))))
    print(f"[lrc] {tag}: AB {e_ab:.2e} (1e-8), mu {e_mu:.2e} (1e-10), err0 {e_e0:.2e} (1e-10), "
          f"orth {e_orth:.2e} (1e-8), rank {info['rank']}")
    assert info["rank"] == ref["rank"] == rank
    assert e_ab <= 1e-8
    assert e_mu <= 1e-10
    assert e_e0 <= 1e-10
    assert e_orth <= 1e-8
    assert abs(info["err1"] - (info["err0"] - info["mu"].sum())) <= 1e-15 * info["err0"]
    # the balancing rule: both factors of a direction within one binade
    for j in range(rank):
        ratio = np.abs(B[j]).max() / np.abs(A[:, j]).max()
        assert 0.5 <= ratio <= 2.0, (j, ratio)
    return AB


@pytest.mark.parametrize("shape,r", L.CASES, ids=L.CASE_IDS)
def test_against_reference(g, shape, r):
    c = L.case(shape, r)
    A, B, info = solve(g, c)
    AB = check_against_reference(f"{shape[0]} r={r}", c, A, B, info)
    direct = L.weighted_error(c["E"].astype(np.float64), AB, c["H"])
    e1 = abs(info["err1"] - direct) / direct
    print(f"[lrc] {shape[0]} r={r}: err1 {info['err1']:.6e} vs direct {direct:.6e}: {e1:.2e} "
          f"(1e-8); err1 / err0 = {info['err1'] / info['err0']:.3e}")
    assert e1 <= 1e-8
    assert info["err1"] <= info["err0"]


F32_CASES = (1, 4, 8, -1)


@pytest.mark.parametrize("shape,r", [L.CASES[i] for i in F32_CASES],
                         ids=[L.CASE_IDS[i] for i in F32_CASES])
def test_float32_outputs_are_the_rounded_float64_ones(g, shape, r):
    c = L.case(shape, r)
    A64, B64, i64 = solve(g, c)
    A32, B32, i32 = solve(g, c, torch.float32)
    assert A32.dtype == B32.dtype == np.float32
    assert bits_equal(A32, A64.astype(np.float32))
    assert bits_equal(B32, B64.astype(np.float32))
    assert bits_equal(i32["mu"], i64["mu"]) and i32["err0"] == i64["err0"]
    # and A B of the stored factors: two roundings to float32 per product
    E = c["E"].astype(np.float64)
    bound = 2.0 ** -23 * (np.abs(A64) @ np.abs(B64))
    assert np.all(np.abs(A32.astype(np.float64) @ B32.astype(np.float64) - A64 @ B64) <= bound)
    assert fro(A32.astype(np.float64) @ B32.astype(np.float64) - A64 @ B64) <= 2.0 ** -23 * fro(E)


def test_rank_deficient_residual(g):
    """E of weighted rank 3, r = 8: rank 3 comes back, the other columns of A
    and rows of B are exactly zero, nothing is NaN."""
    c = L.rank3_case()
    A, B, info = solve(g, c)
    check_against_reference("rank 3, r = 8", c, A, B, info, rank=3)
    assert not A[:, 3:].any() and not B[3:].any() and not info["mu"][3:].any()
    assert abs(info["err1"]) <= 1e-10 * info["err0"]      # everything is captured
    A32, B32, _ = solve(g, c, torch.float32)
    assert np.isfinite(A32).all() and np.isfinite(B32).all() and not A32[:, 3:].any()


def test_zero_residual(g):
    c = dict(L.rank3_case())
    c["E"] = np.zeros_like(c["E"])
    A, B, info = solve(g, c)
    assert info["rank"] == 0 and not A.any() and not B.any() and not info["mu"].any()
    assert info["err0"] == 0.0


def test_dead_and_duplicated_channels(g):
    c = L.degenerate_case()
    A, B, info = solve(g, c)
    AB = check_against_reference("dead + duplicated H", c, A, B, info)
    direct = L.weighted_error(c["E"].astype(np.float64), AB, c["H"])
    assert abs(info["err1"] - direct) <= 1e-8 * direct


def test_sketch_route_matches_gram(g):
    """factor = the float32 sketch Y against gram = 1 with H = Y^T Y."""
    c = L.sketch_case()
    A, B, info = solve(g, c)
    check_against_reference("sketch", c, A, B, info)
    cg = dict(c, kind="gram")
    Ag, Bg, ig = solve(g, cg)
    err = fro(A @ B - Ag @ Bg) / fro(c["E"])
    print(f"[lrc] sketch vs gram: AB {err:.2e} (1e-8)")
    assert err <= 1e-8
    assert abs(info["err0"] - ig["err0"]) <= 1e-10 * ig["err0"]


def padded(a, extra, fill):
    """A view of `a` inside a wider, sentinel-filled allocation."""
    t = torch.full((a.shape[0], a.shape[1] + extra), fill, dtype=a.dtype, device=DEV)
    t[:, :a.shape[1]] = a
    return t, t[:, :a.shape[1]]


@pytest.mark.parametrize("idx", [4, 7, 1], ids=["m-route", "p-route", "gram"])
def test_padded_strides(g, lib, idx):
    """Every matrix with a row stride above its width: the result equals the
    contiguous call bit for bit and the padding keeps its sentinel."""
    shape, r = L.CASES[idx]
    c = L.case(shape, r)
    m, n = c["E"].shape
    want_A, want_B, want = solve(g, c)
    gram = int(c["kind"] == "gram")
    F = dev(c["H"]) if gram else dev(c["F"][:, c["perm"]])
    perm = None if gram else dev(c["perm"])
    p = F.shape[0]
    Eb, E = padded(dev(c["E"]), 3, 7.0)
    Fb, Fv = padded(F, 5, 7.0)
    Ab, A = padded(torch.zeros((m, r), dtype=torch.float64, device=DEV), 2, -3.0)
    Bb, B = padded(torch.zeros((r, n), dtype=torch.float64, device=DEV), 7, -3.0)
    out = torch.empty(r + 1, dtype=torch.float64, device=DEV)
    rank = torch.empty(1, dtype=torch.int32, device=DEV)
    ws = lib.workspace(lib.lib.tg_lrc_workspace_size(m, n, p, r, gram), torch.device(DEV))
    lib.call("tg_lrc_factor", lib.stream(), lib.ptr(E), m, n, E.stride(0), lib.ptr(Fv),
             lib.TG_F64, p, Fv.stride(0), lib.ptr(perm), gram, r, lib.ptr(A), A.stride(0),
             lib.ptr(B), B.stride(0), lib.TG_F64, lib.ptr(out), lib.ptr(out[r:]), lib.ptr(rank),
             lib.ptr(ws), ws.numel())
    torch.cuda.synchronize()
    assert bits_equal(A.cpu().numpy(), want_A) and bits_equal(B.cpu().numpy(), want_B)
    assert bits_equal(out[:r].cpu().numpy(), want["mu"]) and int(rank.item()) == want["rank"]
    assert torch.all(Ab[:, r:] == -3.0) and torch.all(Bb[:, n:] == -3.0)
    assert torch.all(Eb[:, n:] == 7.0) and torch.all(Fb[:, F.shape[1]:] == 7.0)
    assert bits_equal(E.cpu().numpy(), c["E"])


@pytest.mark.parametrize("idx", [5, 8, 17], ids=["m-route", "p-route", "gram-320"])
def test_deterministic(g, idx):
    shape, r = L.CASES[idx]
    c = L.case(shape, r)
    A1, B1, i1 = solve(g, c)
    A2, B2, i2 = solve(g, c)
    assert bits_equal(A1, A2) and bits_equal(B1, B2) and bits_equal(i1["mu"], i2["mu"])
    assert i1["err0"] == i2["err0"] and i1["rank"] == i2["rank"]


def test_workspace_too_small_is_rejected(lib):
    one = ctypes.c_void_p(256)
    rc = lib.lib.tg_lrc_factor(None, one, 8, 16, 16, one, lib.TG_F64, 4, 16, None, 0, 4, one, 4,
                               one, 16, lib.TG_F32, one, one, one, one, 64)
    assert rc == -99
