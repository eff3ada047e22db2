"""CPU proof that tests/test_gpu_degenerate.py is not vacuous: the reference
alone (oracle/oracle.py, LAPACK) meets every bar that file sets, on the inputs
of tests/degenerate_ref.py.  A failure of the GPU file is then a finding about
the HIP code, not about the test.
"""
import numpy as np
import pytest

import degenerate_ref as D


@pytest.fixture(scope="module")
def solved(oracle_mod):
    """case -> (H, factor, Wq, Wrtn); the oracle's whole solve, once per case."""
    cache = {}

    def get(case):
        if case not in cache:
            n, m, nd, npair, bits, group, sym, rule, thr = case
            X, dead, pairs, W = D.pipe_inputs(case)
            H = D.hessian(X, pairs)
            f = oracle_mod.process_hessian_alt(H, thr, rule)
            Wq, _ = oracle_mod.gptq_fwrd(W, f.U, f.perm, bits, group, sym, D.PIPE_BLOCK,
                                         gemm="fma", impl="c")
            cache[case] = (H, f, Wq, D.rtn(W, bits, group, sym))
        return cache[case]
    return get


def test_degenerate_x_structure():
    X, dead, pairs = D.degenerate_x(300, 256, 9, 6, 3)
    assert X.dtype == np.float16 and X.shape == (300, 256)
    assert len(dead) == 9 and len(pairs) == 6 and np.all(np.diff(dead) > 0)
    used = list(dead) + [i for p in pairs for i in p]
    assert len(set(used)) == 9 + 12
    assert not X[:, dead].any()
    for a, b in pairs:
        assert np.array_equal(X[:, a], X[:, b]) and X[:, a].any()
    # scattered, not one contiguous run
    assert np.max(np.diff(np.sort(used))) > 1


@pytest.mark.parametrize("case", D.PIPE_CASES, ids=D.PIPE_IDS)
def test_reference_meets_the_pipeline_bars(oracle_mod, solved, case):
    n, m, nd, npair, bits, group, sym, rule, thr = case
    X, dead, pairs, W = D.pipe_inputs(case)
    assert X.shape == (3 * n // 2, n)
    H, f, Wq, Wrtn = solved(case)
    assert not H[dead].any() and not H[:, dead].any()
    assert np.array_equal(H, H.T)
    for a, b in pairs:
        assert np.array_equal(H[a], H[b]) and np.array_equal(H[:, a], H[:, b])
    k = D.structural_rank(n, dead, pairs)
    assert f.k == k == n - nd - npair
    for fac in (1 - 1e-6, 1 + 1e-6):   # the rank does not hinge on the threshold
        assert oracle_mod.truncation_rank(f.S, thr * fac, rule) == k, "knife-edge input"
    lam = f.S ** 2
    print(f"k={k}, smallest kept eigenvalue {lam[k - 1]:.3e}, largest dropped {lam[k]:.3e}")
    assert np.all(f.S[k:] == 1e-6)                       # the clamp, exactly
    D.check_perm(f.perm, k, n, dead, pairs)
    U_ref, Rx_ref = D.factors_given_perm(H, k, f.perm)
    eu, er = D.rel(f.U, U_ref), D.rel(f.R_x, Rx_ref)
    print(f"factors_given_perm vs oracle: U {eu:.2e}, R_x {er:.2e}")
    assert eu <= 1e-12 and er <= 1e-12
    assert np.array_equal(Wq[:, dead].view(np.uint32), Wrtn[:, dead].view(np.uint32))
    e_solve = oracle_mod.relative_prediction_error(W, Wq, f.R_x, f.perm)
    e_rtn = oracle_mod.relative_prediction_error(W, Wrtn, f.R_x, f.perm)
    print(f"prediction error: solve {e_solve:.4f}, rtn {e_rtn:.4f}")
    assert e_solve < e_rtn


def test_factors_given_perm_is_the_cholesky_form(solved):
    """U^T U = P^T H_k^+ P: the given-perm U equals the upper Cholesky factor of
    the permuted pseudo-inverse's leading block extended by its solve."""
    case = D.PIPE_CASES[0]
    n = case[0]
    H, f, _, _ = solved(case)
    k = f.k
    U_ref, _ = D.factors_given_perm(H, k, f.perm)
    L, V = np.linalg.eigh(H)
    Vk, Lk = V[:, ::-1][:, :k], L[::-1][:k]
    Pinv = (Vk / Lk) @ Vk.T
    Pp = Pinv[f.perm][:, f.perm]
    # U^T U = Pp with U upper trapezoidal: U11 from the leading block, U12 by a solve
    U11 = np.linalg.cholesky(Pp[:k, :k]).T
    U12 = np.linalg.solve(U11.T, Pp[:k, k:])
    err = D.rel(np.hstack([U11, U12]), U_ref)
    print(f"Cholesky form vs QR form: {err:.2e}")
    assert err <= 1e-10


def test_mx_reference_on_the_degenerate_case(solved):
    """The E2M1 solve with the oracle's U / perm: dead columns are plain MX
    casting, and the solve beats plain casting."""
    import mx_ref as R
    case = D.PIPE_CASES[1]
    X, dead, pairs, W = D.pipe_inputs(case)
    H, f, _, _ = solved(case)
    Wq = R.gptq_fwrd_mx(W, f.U.astype(np.float32), f.perm, D.PIPE_BLOCK, False)[0]
    Wc = R.rtn(W)[0]
    assert np.array_equal(Wq[:, dead].view(np.uint32), Wc[:, dead].view(np.uint32))
    from oracle import oracle as o
    e_solve = o.relative_prediction_error(W, Wq, f.R_x, f.perm)
    e_rtn = o.relative_prediction_error(W, Wc, f.R_x, f.perm)
    print(f"mx prediction error: solve {e_solve:.4f}, casting {e_rtn:.4f}")
    assert e_solve < e_rtn


@pytest.mark.parametrize("case", D.PIVOT_CASES, ids=lambda c: "n%d-d%d-p%d" % c)
def test_pivot_cases_are_tie_free(case):
    """Outside the exact ties of the duplicates, the chosen Schur diagonal
    leads the runner-up by >= MIN_GAP at every step, so `perm identical` is a
    fair demand of the GPU's pivot stage."""
    from test_gpu_pivot_levels import MIN_GAP, _min_gap
    H, k, order, Rx_ref, dead, pairs = D.pivot_case(case)
    n = H.shape[0]
    assert k == n - len(dead) - len(pairs)
    gap = _min_gap(H, k, order, Rx_ref, True)
    print(f"{case}: min relative pivot gap {gap:.2e}")
    assert gap >= MIN_GAP
    D.check_perm(order, k, n, dead, pairs)
    assert np.isfinite(Rx_ref).all()


@pytest.mark.parametrize("name", list(D.EIGH_X))
def test_eigh_cases_reach_the_first_panel(name):
    """The first 32-column panel of the band reduction holds an exactly zero
    column, an exactly repeated one, or both: its Gram matrix is singular."""
    n, nd, npair, _ = D.EIGH_X[name]
    X, dead, pairs = D.eigh_x(name)
    H = D.EIGH_CASES[name]
    assert H.shape == (n, n) and len(dead) == nd and len(pairs) == npair
    if nd:
        assert (dead < 32).any()
        assert not H[32:, dead[dead < 32]].any()
    if npair:
        first = [(a, b) for a, b in pairs if a < 32 and b < 32]
        assert first
        a, b = first[0]
        assert np.array_equal(H[32:, a], H[32:, b]) and H[32:, a].any()
    assert np.linalg.matrix_rank(H[32:, :32]) < 32


@pytest.mark.parametrize("name", D.EIGH_NAMES)
def test_lapack_meets_the_eigh_bars(name):
    H = D.EIGH_CASES[name]
    w, V = np.linalg.eigh(H)
    fig = D.check_eigh(name, H, w, V.T[::-1])
    print(f"{name}: {fig}")
