"""GPU: the rotation is only pre- and post-processing of the solver.
``gptq_fwrd`` on ``rows(W)`` with the factor of ``hessian_(H)`` gives codes, scales
and Wq' bit-equal to the existing API called on the host restatement's W' and H'
(had_ref.py) uploaded by hand; the sketch route ``rows(Y)`` equals the
restatement on Y; and the quality case of test_had_ref.py holds on the GPU.

The integer grid uses groups of 128 where 128 divides n (32 x 256) and groups of
32 at n = 160, which 128 does not divide (``Quantizer`` takes whole groups only)."""
import numpy as np
import pytest
import torch

import had_ref as hr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(17, 160, 32), (32, 256, 128)]       # m, n, block


@pytest.fixture(scope="module")
def g():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gptq_svd_amd.gptq_utils as g
    return g


def quantizer(g, fmt, n):
    if fmt == "mxfp4":
        return g.Quantizer(4, 32, False, weight_format="mxfp4")
    return g.Quantizer(4, 128 if n % 128 == 0 else 32, False)


def solve(g, W, H, mode, fmt):
    """(Wq, (codes, E8M0 bytes or None), scale, zero, k) of the existing API on device
    tensors.  The codes are compared unpacked: 17 rows do not fill whole words."""
    if mode == "eigh":
        R, R_x, perm = g.process_hessian_alt(H, 1e-4, "energy")
    else:
        R, perm = g.process_hessian(H, actorder=False, damp_percent=0.01)
        R_x = None
    q = quantizer(g, fmt, W.shape[1])
    Wq, k = g.gptq_fwrd(W, R, q, perm, block_size=1024, use_triton=(mode == "eigh"), R_x=R_x)
    return Wq, (q.codes, q.scale_e8m0), q.scale, q.zero, k


@pytest.fixture(scope="module")
def cases():
    from mx_ref import hessian_case
    out = {}
    for m, n, b in SHAPES:
        W = hr.outlier_weight(m, n, seed=n)
        H = hessian_case(n, 4 * n, 1)
        words = hr.pack_signs(hr.mixed_signs(n, b, 3))
        out[(m, n, b)] = (W, H, words, hr.rows_np(W, b, words), hr.sym(H, b, words))
    return out


@pytest.mark.parametrize("mode", ["eigh", "gptq"])
@pytest.mark.parametrize("fmt", ["int", "mxfp4"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}b{s[2]}")
def test_rotated_solve_is_the_plain_solve_on_the_restatement(g, cases, shape, fmt, mode):
    m, n, b = shape
    W, H, words, Wr, Hr = cases[shape]
    rot = g.HadamardRotation(n, b, sign_bits=torch.from_numpy(words), device=DEV)
    Wd = rot.rows(torch.from_numpy(W).to(DEV))
    Hd = rot.hessian_(torch.from_numpy(H).to(DEV))
    assert np.array_equal(hr.raw_bits(Wd), hr.raw_bits(torch.from_numpy(Wr)))
    assert np.array_equal(hr.raw_bits(Hd), hr.raw_bits(torch.from_numpy(Hr)))
    got = solve(g, Wd, Hd, mode, fmt)
    want = solve(g, torch.from_numpy(Wr).to(DEV), torch.from_numpy(Hr).to(DEV), mode, fmt)
    assert got[4] == want[4]
    assert torch.equal(got[0], want[0])
    for a, c in zip(got[1], want[1]):
        assert (a is None and c is None) or torch.equal(a, c)
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
    # and back: the write-back is R^-1 of Wq' as the restatement computes it
    back = rot.rows(got[0].float(), inverse=True)
    ref = hr.rows(got[0].float().cpu(), b, words, inverse=True)
    assert np.array_equal(hr.raw_bits(back), hr.raw_bits(ref))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}b{s[2]}")
def test_sketch_route(g, shape):
    """rows(Y) on a scaled sketch (p x n float32) is the restatement on Y."""
    m, n, b = shape
    Y = torch.randn(4 * n + 3, n, generator=torch.Generator().manual_seed(n))
    rot = g.HadamardRotation(n, b, seed=11, device=DEV)
    got = rot.rows(Y.to(DEV))
    assert got.dtype == torch.float32
    want = hr.rows(Y, b, rot.sign_bits.cpu().numpy())
    assert np.array_equal(hr.raw_bits(got), hr.raw_bits(want))
    # (Y Q)^T (Y Q) = Q^T (Y^T Y) Q
    Q = hr.q_matrix(n, b, rot.sign_bits.cpu().numpy())
    G = Y.double().numpy().T @ Y.double().numpy()
    Gr = got.double().cpu().numpy().T @ got.double().cpu().numpy()
    assert np.linalg.norm(Gr - Q.T @ G @ Q) <= 1e-5 * np.linalg.norm(G)


def test_quality_case(g):
    """The case test_had_ref.py proves a factor 4 on with the oracle: on the GPU
    the rotated weighted error is below half of the unrotated one."""
    q = hr.QUALITY
    W, H, words = hr.quality_case()
    Wd, Hd = torch.from_numpy(W).to(DEV), torch.from_numpy(H).to(DEV)
    Wq = solve(g, Wd, Hd.clone(), "eigh", "int")[0]
    plain = hr.weighted_error(W, Wq.float().cpu().numpy(), H)
    rot = g.HadamardRotation(q["n"], q["b"], sign_bits=torch.from_numpy(words), device=DEV)
    Wr, Hr = rot.rows(Wd), rot.hessian_(Hd.clone())
    Wqr = solve(g, Wr, Hr.clone(), "eigh", "int")[0]
    rotated = hr.weighted_error(Wr.cpu().numpy(), Wqr.float().cpu().numpy(), Hr.cpu().numpy())
    # the same number in the original basis (the objective is invariant)
    back = rot.rows(Wqr.float(), inverse=True)
    orig = hr.weighted_error(W, back.cpu().numpy(), H)
    print(f"[had solver] weighted error {plain:.4e} unrotated, {rotated:.4e} rotated "
          f"({orig:.4e} in the original basis), ratio {plain / rotated:.2f}")
    assert abs(orig - rotated) <= 1e-4 * rotated
    assert rotated < 0.5 * plain
