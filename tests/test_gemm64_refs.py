"""CPU: the references and checks of test_gpu_gemm64_family.py check themselves.

The chunk reference is compared with plain scalar loops, and a numpy emulation
of a tiled kernel shows that the comparisons the GPU tests make would notice a
subtly wrong kernel: a dropped last k-slab, a tile that is not mirrored, and a
write into the padding of C each fail them, while the faultless emulation
passes."""
import numpy as np
import pytest

import gemm64_refs as R


def ints(rng, shape, lim=3):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)


# (ta, tb, spec as the GPU test builds it from lda / ldb / ldc, shapes of A, B, C)
def tiny_specs(lda, ldb, ldc):
    return {
        "nn_k": (0, 0, [4, 3, 11, 1, 0, ldb, 0, 0, 3, 5, 3, -1], (5, 11), (11, 3), (5, 9)),
        "tn_partials": (1, 0, [2, 3, 6, 3 * lda, 0, ldb, 0, 0, 5 * ldc, 5, 2, 2], (14, 5), (6, 2),
                        (15, 2)),
        "tn_k": (1, 0, [4, 2, 7, lda, 0, ldb, 0, 0, 2, 5, 2, -1], (7, 5), (7, 2), (5, 4)),
        "nt_m": (0, 1, [4, 2, 7, lda, 0, 0, 2, ldc, 0, -1, 5, 2], (7, 2), (5, 4), (7, 5)),
    }


@pytest.mark.parametrize("name", ["nn_k", "tn_partials", "tn_k", "nt_m"])
@pytest.mark.parametrize("layout", ["C", "B", "V"])
@pytest.mark.parametrize("beta", [0.0, -0.25])
def test_chunk_reference_equals_scalar_loops(name, layout, beta):
    rng = np.random.default_rng(5)
    shapes = tiny_specs(0, 0, 0)[name][3:]
    (la, lda), (lb, ldb), (lc, ldc) = (R.place(s[1], layout) for s in shapes)
    ta, tb, spec, sa, sb, sc = tiny_specs(lda, ldb, ldc)[name]
    Af, Bf = R.flat_image(ints(rng, sa), lda, la), R.flat_image(ints(rng, sb), ldb, lb)
    C0 = R.flat_image(ints(rng, sc, 8), ldc, lc)
    got, want = C0.copy(), C0.copy()
    R.chunked_apply(ta, tb, spec, 0.5, Af, la, lda, Bf, lb, ldb, beta, got, lc, ldc)
    R.chunked_loops(ta, tb, spec, 0.5, Af, la, lda, Bf, lb, ldb, beta, want, lc, ldc)
    assert R.first_mismatch(got, want) is None
    # every chunk wrote something, and only inside the logical C
    assert not np.array_equal(got, C0)
    keep = C0.copy()
    R.view(keep, lc, *sc, ldc)[...] = R.view(got, lc, *sc, ldc)
    assert R.first_mismatch(got, keep) is None


def test_chunks_follow_the_header():
    # c = 4, nc = 3, m = 11: chunks of 4, 4 and the remaining 3; negative M / N / K = the length
    assert R.chunks([4, 3, 11, 0, 0, 0, 0, 0, 0, -1, 7, -1]) == [
        (0, 0, 4, 4, 7, 4), (1, 4, 4, 4, 7, 4), (2, 8, 3, 3, 7, 3)]
    # the last chunk takes whatever is left, more than c included
    assert R.chunks([4, 2, 11, 0, 0, 0, 0, 0, 0, 2, 2, -1])[-1] == (1, 4, 7, 2, 2, 7)


@pytest.mark.parametrize("fault", [None, "drop_slab", "no_mirror", "pad_write"])
@pytest.mark.parametrize("mode", ["exact", "bounded"])
def test_the_checks_notice_an_injected_fault(fault, mode):
    """A SYRK C = alpha X^T X + beta C0 of 130 columns over K = 40 through the
    emulation; the three checks of the GPU tests (flat image against the
    reference, symmetry bit for bit, the numerics bound) must pass without a
    fault and at least one of them must fail with each."""
    rng = np.random.default_rng(11)
    n, K, alpha, beta = 130, 40, 0.5, -0.25
    X = ints(rng, (K, n)) if mode == "exact" else rng.standard_normal((K, n))
    C0 = ints(rng, (n, n), 8) if mode == "exact" else rng.standard_normal((n, n))
    C0 = np.tril(C0) + np.tril(C0, -1).T
    lead, ldc = R.place(n, "B")
    before = R.flat_image(C0, ldc, lead)
    after = R.emulate(before.copy(), lead, ldc, n, n, alpha, X.T, X, beta, fault=fault, syrk=True)
    want = before.copy()
    if mode == "exact":
        R.view(want, lead, n, n, ldc)[...] = R.gemm_exact(1, 0, alpha, X, X, beta, C0)
        ok = R.first_mismatch(after, want) is None
    else:
        ref, bound = R.gemm_bound(1, 0, alpha, X, X, beta, C0)
        got = R.view(after, lead, n, n, ldc)
        ok = R.worst_ratio(got, ref, bound) <= 1.0
        R.view(want, lead, n, n, ldc)[...] = got     # the padding check of the bounded tests
        ok = ok and R.first_mismatch(after, want) is None
    got = R.view(after, lead, n, n, ldc)
    ok = ok and np.array_equal(got, got.T)
    assert ok == (fault is None)


def test_worst_ratio_and_poison():
    ref = np.array([[1.0, 2.0]])
    assert R.worst_ratio(ref.copy(), ref, np.zeros_like(ref)) == 0.0       # 0 / 0
    assert R.worst_ratio(ref + [[0.0, 1e-3]], ref, np.full_like(ref, 1e-3)) == pytest.approx(1.0)
    assert R.worst_ratio(np.array([[np.nan, 2.0]]), ref, np.ones_like(ref)) == np.inf
    T = R.tri_nan(np.ones((5, 5)), 2)
    # zeros inside the 2 x 2 diagonal blocks, NaN strictly below them
    assert T[1, 0] == 0.0 and T[3, 2] == 0.0 and np.isnan(T[2, 1]) and np.isnan(T[4, 0])
    assert np.array_equal(np.triu(T), np.triu(np.ones((5, 5))))
    assert R.syrk_lower_mask(130)[0, 63] and not R.syrk_lower_mask(130)[63, 64]
    assert R.syrk_lower_mask(130)[64, 0] and R.syrk_lower_mask(130)[129, 129]
