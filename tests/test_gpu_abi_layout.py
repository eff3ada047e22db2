"""The FP64 chain of the C ABI with ld != width and bases that are not the
start of an allocation (include/truncgptq.h: "plain device pointers with
explicit leading dimensions").

One problem, n = 333 (odd, no multiple of any tile): H = X^T X / 250 from 250
Gaussian rows, so rank 250 and the mean-trimmed rule at 5e-4 keeps k = 250 < n.
Every stage runs in three layouts (abi_helpers.LAYOUTS):

  C  contiguous;
  A  ld = width + 8: padded, every row still 16-byte aligned;
  B  one element into the allocation, ld = width + 3: no 16-byte alignment,
     which sends every gated 16-byte load to its 8-byte form.

Bars, all stated elsewhere in the project: eigenvalues, residual and
orthogonality as tests/test_gpu_solver.py::test_eigh; perm identical to LAPACK
dgeqp3's, S within 1e-12, U and R_x within 1e-8 relative Frobenius of the
oracle (test_process_hessian_alt_golden); the comparator factor within 1e-9 of
the oracle and R^T R (H_p + damp I) = I to 1e-9 (tests/test_gpu_gptq.py); the
band stage's eigenvalues within 1e-12 ||B|| (tests/test_gpu_bulge.py).  Around
every output the lead-in, the columns width .. ld-1 and the tail must still
hold the sentinel; inputs must come back unchanged.

The pivot order can only be compared where the input has no near-tie:
test_pivot_input_is_tie_free checks that on the CPU, from the oracle's
numbers alone.
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sl
import torch

from abi_helpers import DEV, LAYOUTS, SENTINEL, dev, lay, logical, outside_intact

N, ROWS, SEED = 333, 250, 333
THRESHOLD, RULE = 5e-4, "mean_trimmed"
TIE_GAP = 1e-8


@pytest.fixture(scope="module")
def lib():
    from gptq_svd_amd import _lib
    return _lib


def hessian():
    X = np.random.default_rng(SEED).standard_normal((ROWS, N))
    return X.T @ X / ROWS


@pytest.fixture(scope="module")
def prob(oracle_mod):
    """H, LAPACK's eigenvalues and the oracle's factor, computed once."""
    H = hessian()
    f = oracle_mod.process_hessian_alt(H, THRESHOLD, RULE)
    return H, np.linalg.eigvalsh(H), f


def pivot_gaps(f):
    """Greedy column pivoting on S_k = diag(S[:k]) Vh_k recovered from the
    oracle's factor (R_x = Q^T S_k P, so the column norms of R_x's trailing
    block are those of the projected S_k): at step j the largest remaining
    column norm and the runner-up.  Returns the relative gaps."""
    R = f.R_x                              # columns already in pivot order
    k = R.shape[0]
    gaps = []
    for j in range(k):
        nrm = np.sort(np.linalg.norm(R[j:, j:], axis=0))[::-1]
        if nrm.size > 1:
            gaps.append((nrm[0] - nrm[1]) / nrm[0])
        # the oracle's own choice must be the largest: column j of the trailing block
        assert np.linalg.norm(R[j:, j]) == pytest.approx(nrm[0], rel=1e-12)
    return np.array(gaps)


def test_pivot_input_is_tie_free(prob):
    """At each of the k greedy steps the best remaining column norm exceeds the
    runner-up by more than 1e-8 relative, so the pivot order is determined far
    above the 1e-8 accuracy of the factors and `perm identical` is a fair
    demand.  (No GPU: a later change of SEED cannot hide a tie.)"""
    H, L, f = prob
    assert f.k == ROWS < N
    gaps = pivot_gaps(f)
    print(f"pivot gaps: min {gaps.min():.2e} over {gaps.size} steps")
    assert gaps.min() > TIE_GAP


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def out_buf(shape, layout, fill=0.0):
    return lay(np.full(shape, fill), layout)


def check_out(tag, buf, shape, ld, lead):
    assert outside_intact(buf, shape, ld, lead), f"{tag}: wrote outside the logical matrix"
    return logical(buf, shape, ld, lead)


def check_in(tag, buf, a, ld, lead):
    assert outside_intact(buf, a.shape, ld, lead), f"{tag}: input padding changed"
    got = logical(buf, a.shape, ld, lead)
    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(a).view(np.uint64)), \
        f"{tag}: input changed"


def check_factor(tag, M, ref, k, tol=1e-8):
    err = rel(M, ref)
    print(f"{tag}: rel {err:.2e}")
    assert err <= tol, tag
    assert np.all(np.tril(M[:, :k], -1) == 0.0), f"{tag}: strict lower triangle not 0"
    assert np.all(np.diag(M[:, :k]) > 0), tag


RESULTS = {}  # layout -> {name: array}; for the bit-identity report


def report_bit_identity(layout):
    if layout == "C" or "C" not in RESULTS:
        return
    for name, a in RESULTS[layout].items():
        b = RESULTS["C"][name]
        same = a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
        print(f"layout {layout} vs C, {name}: {'bit-identical' if same else 'differs'}")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_fp64_chain(lib, prob, layout):
    H, L, f = prob
    n, k = N, f.k
    nc = n - k
    st = lib.stream()
    nrm = np.abs(L).max()
    res = RESULTS.setdefault(layout, {})

    # 1. eigenvalues (A is destroyed, its surroundings are not)
    pA, bA, lda, leadA = lay(H, layout)
    ws = lib.workspace(lib.lib.tg_eigh_workspace_size(n), DEV)
    w = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    lib.call("tg_eigh_values", st, pA, n, lda, lib.ptr(w), lib.ptr(ws), ws.numel())
    assert outside_intact(bA, H.shape, lda, leadA), "tg_eigh_values wrote outside A"
    wh = w.cpu().numpy()
    assert wh[n] == SENTINEL
    wh = res["w"] = wh[:n].copy()
    assert np.max(np.abs(wh - L)) <= 1e-12 * nrm * max(1, np.sqrt(n) / 8)

    # rank and S from the library's own eigenvalues
    S = torch.empty(n, dtype=torch.float64, device=DEV)
    kd = torch.empty(1, dtype=torch.int32, device=DEV)
    lib.call("tg_truncation_rank", st, lib.ptr(w), n, THRESHOLD, lib.RULES[RULE], lib.ptr(S),
             lib.ptr(kd))
    assert int(kd.item()) == k
    assert rel(S.cpu().numpy(), f.S) < 1e-12

    # 2. kept eigenvectors, and the dropped ones for the complement path
    pV, bV, ldv, leadV = out_buf((k, n), layout)
    lib.call("tg_eigh_vectors_range", st, n, lib.ptr(w), 0, k, pV, ldv, lib.ptr(ws), ws.numel())
    Vh = res["Vh"] = check_out("Vh", bV, (k, n), ldv, leadV)
    lam = wh[::-1][:k]
    assert np.linalg.norm(Vh @ H - lam[:, None] * Vh, axis=1).max() <= 1e-10 * nrm
    assert np.abs(Vh @ Vh.T - np.eye(k)).max() <= 1e-10
    pVc, bVc, ldvc, leadVc = out_buf((nc, n), layout)
    lib.call("tg_eigh_vectors_range", st, n, lib.ptr(w), k, nc, pVc, ldvc, lib.ptr(ws),
             ws.numel())
    Vc = check_out("Vc", bVc, (nc, n), ldvc, leadVc)
    assert np.all(np.isfinite(Vc))
    # the dropped eigenvalues are one cluster at zero: any basis of the null
    # space serves, so only its residual is held to the eigenvector bar
    assert np.linalg.norm(Vc @ H - wh[::-1][k:, None] * Vc, axis=1).max() <= 1e-10 * nrm
    del ws

    # 3. pivot order and R_x, kept form
    perm = torch.full((n + 1,), -5, dtype=torch.int64, device=DEV)
    pR, bR, ldr, leadR = out_buf((k, n), layout)
    pws = lib.workspace(lib.lib.tg_pivot_workspace_size(n, k), DEV)
    lib.call("tg_pivoted_factor", st, pV, ldv, lib.ptr(S), n, k, lib.ptr(perm), pR, ldr,
             lib.ptr(pws), pws.numel())
    ph = perm.cpu().numpy()
    assert ph[n] == -5 and np.array_equal(ph[:n], f.perm)
    Rx = res["Rx"] = check_out("R_x", bR, (k, n), ldr, leadR)
    check_factor(f"layout {layout} R_x (kept)", Rx, f.R_x, k)
    check_in("Vh after tg_pivoted_factor", bV, Vh, ldv, leadV)

    # ... and the complement form: H_k = H - B_c^T B_c
    pH, bH, ldh, leadH = lay(H, layout)
    perm2 = torch.full((n + 1,), -5, dtype=torch.int64, device=DEV)
    pR2, bR2, ldr2, leadR2 = out_buf((k, n), layout)
    Sc = ctypes.c_void_p(S.data_ptr() + 8 * k)
    lib.call("tg_pivoted_factor_complement", st, pH, ldh, pVc, ldvc, Sc, nc, n, k, lib.ptr(perm2),
             pR2, ldr2, lib.ptr(pws), pws.numel())
    ph2 = perm2.cpu().numpy()
    assert ph2[n] == -5 and np.array_equal(ph2[:n], f.perm)
    Rx2 = res["Rx_complement"] = check_out("R_x (complement)", bR2, (k, n), ldr2, leadR2)
    check_factor(f"layout {layout} R_x (complement)", Rx2, f.R_x, k)
    check_in("H after tg_pivoted_factor_complement", bH, H, ldh, leadH)
    check_in("Vc after tg_pivoted_factor_complement", bVc, Vc, ldvc, leadVc)
    del pws

    # 4. U, both forms
    pU, bU, ldu, leadU = out_buf((k, n), layout, fill=3.5)
    uws = lib.workspace(lib.lib.tg_ufactor_workspace_size(n, k), DEV)
    lib.call("tg_u_factor", st, pV, ldv, lib.ptr(S), lib.ptr(perm), n, k, pU, ldu, lib.ptr(uws),
             uws.numel())
    U = res["U"] = check_out("U", bU, (k, n), ldu, leadU)
    check_factor(f"layout {layout} U (kept)", U, f.U, k)
    check_in("Vh after tg_u_factor", bV, Vh, ldv, leadV)
    pU2, bU2, ldu2, leadU2 = out_buf((k, n), layout, fill=3.5)
    uws = lib.workspace(lib.lib.tg_ufactor_rx_workspace_size(n, k), DEV)
    lib.call("tg_u_factor_rx", st, pR2, ldr2, n, k, pU2, ldu2, lib.ptr(uws), uws.numel())
    U2 = res["U_complement"] = check_out("U (complement)", bU2, (k, n), ldu2, leadU2)
    check_factor(f"layout {layout} U (complement)", U2, f.U, k)
    check_in("R_x after tg_u_factor_rx", bR2, Rx2, ldr2, leadR2)
    report_bit_identity(layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_urx_pieces(lib, prob, layout):
    """tg_urx_c in two column blocks into one padded C, tg_urx_u11 from it, and
    tg_urx_u12 per block straight into U's columns k + c0 .. (ldo = ldu)."""
    H, L, f = prob
    n, k = N, f.k
    m = n - k
    assert m * 16 > k  # the explicit form
    st = lib.stream()
    blocks = [(0, 40), (40, m)]
    pR, bR, ldr, leadR = lay(f.R_x, layout)
    pC, bC, ldc, leadC = out_buf((k, m), layout)
    pU, bU, ldu, leadU = out_buf((k, n), layout)
    ws = lib.workspace(lib.lib.tg_ufactor_rx_workspace_size(n, k), DEV)
    for c0, c1 in blocks:
        lib.call("tg_urx_c", st, pR, ldr, n, k, c0, c1, ctypes.c_void_p(pC.value + 8 * c0), ldc,
                 lib.ptr(ws), ws.numel())
    C = check_out("C", bC, (k, m), ldc, leadC)
    R11, R12 = f.R_x[:, :k], f.R_x[:, k:]
    assert rel(C, sl.solve_triangular(R11, R12)) <= 1e-8
    lib.call("tg_urx_u11", st, pR, ldr, n, k, pC, ldc, pU, ldu, lib.ptr(ws), ws.numel())
    for c0, c1 in blocks:
        lib.call("tg_urx_u12", st, pU, ldu, k, ctypes.c_void_p(pC.value + 8 * c0), ldc, c1 - c0,
                 ctypes.c_void_p(pU.value + 8 * (k + c0)), ldu)
    U = check_out("U", bU, (k, n), ldu, leadU)
    check_factor(f"layout {layout} U (urx pieces)", U, f.U, k)
    check_in("R_x", bR, f.R_x, ldr, leadR)
    check_in("C after u11 / u12", bC, C, ldc, leadC)
    # the header's claim for the pieces: tg_u_factor_rx's U bit for bit
    dR = dev(f.R_x)
    full = torch.empty((k, n), dtype=torch.float64, device=DEV)
    lib.call("tg_u_factor_rx", st, lib.ptr(dR), n, n, k, lib.ptr(full), n, lib.ptr(ws), ws.numel())
    same = np.array_equal(full.cpu().numpy().view(np.uint64), U.view(np.uint64))
    print(f"layout {layout}: pieces vs one tg_u_factor_rx call: "
          f"{'bit-identical' if same else 'differs'}")


@pytest.mark.gpu
@pytest.mark.parametrize("actorder", [False, True], ids=["perm-null", "perm-given"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_hinv_chol_layout(lib, oracle_mod, prob, layout, actorder):
    H, L, f = prob
    n = N
    R_ref, perm, rung = oracle_mod.process_hessian(H, actorder=actorder, damp_percent=0.01)
    assert rung == 0
    pH, bH, ldh, leadH = lay(H, layout)
    pR, bR, ldr, leadR = out_buf((n, n), layout, fill=3.5)
    dperm = dev(perm.astype(np.int64)) if actorder else None
    tries = ctypes.c_int(-1)
    ws = lib.workspace(lib.lib.tg_hinv_chol_workspace_size(n), DEV)
    lib.call("tg_hinv_chol", lib.stream(), pH, n, ldh, lib.ptr(dperm), 0.01, 5, pR, ldr,
             ctypes.byref(tries), lib.ptr(ws), ws.numel())
    assert tries.value == rung
    R = check_out("R", bR, (n, n), ldr, leadR)
    check_in("H", bH, H, ldh, leadH)
    check_factor(f"layout {layout} hinv_chol actorder={actorder}", R, R_ref, n, tol=1e-9)
    Hp = H[perm][:, perm] + 0.01 * np.mean(np.diag(H)) * np.eye(n)
    assert np.abs(R.T @ R @ Hp - np.eye(n)).max() <= 1e-9


def band_matrix(n, seed, b=32):
    rng = np.random.default_rng(seed)
    A = np.zeros((n, n))
    for dg in range(b + 1):
        v = rng.standard_normal(n - dg)
        A[np.arange(dg, n), np.arange(n - dg)] = v
        A[np.arange(n - dg), np.arange(dg, n)] = v
    return A


@pytest.mark.gpu
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_band_tridiag_layout(lib, layout):
    """Only the lower band is read: everything else of A holds the sentinel."""
    n, b = N, 32
    B = band_matrix(n, n)
    i, j = np.indices((n, n))
    A = np.where((i >= j) & (i - j <= b), B, SENTINEL)
    pA, bA, lda, leadA = lay(A, layout)
    ws = lib.workspace(lib.lib.tg_band_tridiag_workspace_size(n), DEV)
    ws.zero_()
    d = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    e = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    lib.call("tg_band_tridiag", lib.stream(), pA, n, lda, lib.ptr(d), lib.ptr(e), lib.ptr(ws),
             ws.numel())
    torch.cuda.synchronize()
    check_in("A", bA, A, lda, leadA)
    d, e = d.cpu().numpy(), e.cpu().numpy()
    assert d[n] == SENTINEL and e[n] == SENTINEL
    ref = sl.eigvalsh(B)
    got = sl.eigvalsh_tridiagonal(d[:n], e[:n - 1])
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"layout {layout} tg_band_tridiag: eigenvalue error {err:.2e} ||B||")
    assert err <= 1e-12
