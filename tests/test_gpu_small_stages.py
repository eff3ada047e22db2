"""The small stages of the C ABI called directly, off the contiguous path:
odd widths, padded leading dimensions, bases that are not 16-byte aligned.

Every bar is one the project already states: bit-exact scale / zero / codes /
dequantised weights against the CPU oracle (tests/test_gpu_quant.py), 1e-5
relative for the prediction-error metric (tests/test_metric.py), identical
rank.  Shapes are the smallest that reach the code in question:

* n % 4 != 0 with several blocks sends the cross-block update of
  tg_gptq_quantize / tg_gptq_quantize_loop to cross_gemm_scalar_kernel
  (every other quantize test has n % 4 == 0);
* tg_pred_error takes metric_gemm_kernel<false> for n % 4 != 0, for an odd
  ldr and for an R_x that is not 16-byte aligned, <true> otherwise;
* tg_truncation_rank: the chunk-of-64 tails of the energy rule, the ref_k
  edges (n = 1, 2, 33, 34) of mean-trimmed, and both sides of the n = 16384
  switch between the LDS and the global kernel.
"""
import ctypes

import numpy as np
import pytest
import torch

from abi_helpers import DEV, SENTINEL, dev, lay, logical, outside_intact, padded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from gptq_svd_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def g():
    import gptq_svd_amd.gptq_utils as g
    return g


def bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


# ---------------------------------------------------------------------------
# tg_gptq_quantize / tg_gptq_quantize_loop with n % 4 != 0
# ---------------------------------------------------------------------------
def random_problem(m, n, k, seed):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((m, n)) * 0.05).astype(np.float32)
    U = np.triu(rng.standard_normal((k, n)) * 0.02)
    U[np.arange(k), np.arange(k)] = 1.0 + np.abs(rng.standard_normal(k))
    perm = rng.permutation(n).astype(np.int64)
    return W, U.astype(np.float32), perm


ODD_SHAPES = [(150, 330, 300, 4, -1, False, 128), (150, 330, 300, 4, 110, False, 128),
              (70, 250, 250, 3, 125, True, 100)]


@pytest.fixture(scope="module")
def odd_refs(oracle_mod):
    """(shape, use_triton) -> (W, U, perm, Wq_ref, codes_ref incl. offset); computed once."""
    cache = {}

    def get(shape, use_triton):
        key = (shape, use_triton)
        if key not in cache:
            m, n, k, bits, group, sym, block = shape
            W, U, perm = random_problem(m, n, k, m + n + k)
            ref, _, codes = oracle_mod.gptq_fwrd(W, U, perm, bits, group, sym, block, gemm="fma",
                                                 impl="c", return_codes=True,
                                                 use_triton=use_triton)
            cache[key] = (W, U, perm, ref, codes + oracle_mod.code_offset(bits, sym))
        return cache[key]
    return get


@pytest.mark.parametrize("use_triton", [True, False], ids=["block", "loop"])
@pytest.mark.parametrize("shape", ODD_SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_gptq_fwrd_odd_width_exact(g, odd_refs, shape, use_triton):
    m, n, k, bits, group, sym, block = shape
    assert n % 4 != 0 and k > block  # the scalar cross-block kernel, more than one block
    W, U, perm, ref, codes = odd_refs(shape, use_triton)
    q = g.Quantizer(bits, group, sym)
    Wq, kk = g.gptq_fwrd(dev(W), dev(U), q, dev(perm), block_size=block, use_triton=use_triton)
    Wq = Wq.cpu().numpy()
    assert kk == k
    assert bits_equal(Wq, ref), f"{np.mean(Wq != ref)} of elements differ"
    assert np.array_equal(q.codes.cpu().numpy().astype(np.int64), codes)


@pytest.mark.parametrize("name", ["tg_gptq_quantize", "tg_gptq_quantize_loop"])
def test_gptq_quantize_padded_ldu(lib, oracle_mod, odd_refs, name):
    """The ABI itself with ldu = n + 3 and a U that starts one element into its
    allocation."""
    shape = ODD_SHAPES[1]
    m, n, k, bits, group, sym, block = shape
    W, U, perm, ref, codes = odd_refs(shape, name == "tg_gptq_quantize")
    scale, zero = oracle_mod.find_params(W, bits, group, sym)
    pU, bufU = padded(U, n + 3, 1)
    dW, dperm, dscale, dzero = dev(W), dev(perm), dev(scale), dev(zero)
    Wq = torch.full((m, n), SENTINEL, dtype=torch.float32, device=DEV)
    cd = torch.full((m, n), 255, dtype=torch.uint8, device=DEV)
    ws = lib.workspace(lib.lib.tg_quantize_workspace_size(m, n, block), DEV)
    lib.call(name, lib.stream(), lib.ptr(dW), m, n, pU, k, n + 3, lib.ptr(dperm), lib.ptr(dscale),
             lib.ptr(dzero), group, bits, int(sym), block, lib.ptr(Wq), lib.ptr(cd), lib.ptr(ws),
             ws.numel())
    assert bits_equal(Wq.cpu().numpy(), ref)
    assert np.array_equal(cd.cpu().numpy().astype(np.int64), codes)
    assert bits_equal(logical(bufU, U.shape, n + 3, 1), U) and outside_intact(bufU, U.shape, n + 3, 1)


# ---------------------------------------------------------------------------
# tg_pred_error
# ---------------------------------------------------------------------------
# (m, k, n, ldw - n, ldr - n, lead of R_x): which gate of metric.hip it is for
METRIC_CASES = {
    "n%4": (150, 300, 330, 3, 0, 0),          # <false>: n
    "odd-ldr": (150, 300, 328, 0, 3, 0),      # <false>: ldr
    "offset-rx": (150, 300, 328, 0, 0, 1),    # <false>: alignment of R_x
    "aligned": (150, 300, 328, 0, 0, 0),      # <true>, ragged m and k
    "aligned-padded": (150, 300, 328, 8, 8, 0),  # <true>, ld != width
    "k=1": (150, 1, 328, 0, 0, 0),
    "m=1": (1, 300, 330, 3, 0, 0),
}


@pytest.mark.parametrize("case", sorted(METRIC_CASES))
def test_pred_error_direct(lib, oracle_mod, case):
    m, k, n, padw, padr, leadr = METRIC_CASES[case]
    rng = np.random.default_rng(m + k + n)
    W = rng.standard_normal((m, n)).astype(np.float32)
    Wq = (W + 0.01 * rng.standard_normal((m, n))).astype(np.float32)
    Rx = np.triu(rng.standard_normal((k, n)))
    perm = rng.permutation(n).astype(np.int64)
    ref = oracle_mod.relative_prediction_error(W, Wq, Rx, perm)
    pW, bW = padded(W, n + padw, 1 if padw else 0)
    pQ, bQ = padded(Wq, n + padw, 1 if padw else 0)
    pR, bR = padded(Rx, n + padr, leadr)
    if case.startswith("aligned"):
        assert n % 4 == 0 and (n + padr) % 2 == 0 and pR.value % 16 == 0
    else:
        assert n % 4 != 0 or (n + padr) % 2 == 1 or pR.value % 16 != 0 or min(m, k) == 1
    dperm = dev(perm)
    out = torch.zeros(2, dtype=torch.float64, device=DEV)
    ws = lib.workspace(lib.lib.tg_pred_error_workspace_size(m, n, k), DEV)
    lib.call("tg_pred_error", lib.stream(), pW, pQ, m, n, n + padw, pR, k, n + padr,
             lib.ptr(dperm), lib.ptr(out), lib.ptr(ws), ws.numel())
    den, num = out.tolist()
    v = (num ** 0.5) / (den ** 0.5)
    print(f"tg_pred_error {case}: {v:.9f} vs oracle {ref:.9f} (rel {abs(v - ref) / ref:.2e})")
    assert abs(v - ref) <= 1e-5 * ref, (v, ref)


# ---------------------------------------------------------------------------
# tg_truncation_rank
# ---------------------------------------------------------------------------
RANK_N = [1, 2, 33, 34, 63, 64, 65, 100, 1000, 16384, 16385, 20001]
# label -> (rule, threshold).  energy-all: a threshold below zero puts the
# target above the total energy, so every partial sum counts and k = n with
# nothing near a tie.  It is the one energy case in which the counting loop
# reaches the last, partial chunk of 64 (with a threshold above zero the count
# stops at the cut, long before it), so it is what notices a miscounted tail.
RANK_CASES = {"energy": ("energy", 1e-4), "energy-all": ("energy", -1e-4),
              "mean_trimmed": ("mean_trimmed", 5e-4), "none": ("none", 0.0)}


def graded_spectrum(n):
    """Ascending eigenvalues over ten decades whose lowest tenth is negative
    (the 1e-12 clamp).  The positive part is jittered: an exactly geometric
    sequence puts the energy rule's target on a partial sum when the decades
    line up (n = 34, 16384, 20001 with 1e-4)."""
    rng = np.random.default_rng(n)
    neg = n // 10
    pos = np.sort(np.logspace(-9, 1, n - neg) * (1.0 + 0.5 * rng.random(n - neg)))
    return np.concatenate([-np.logspace(-3, -9, neg), pos])


@pytest.mark.parametrize("case", sorted(RANK_CASES))
@pytest.mark.parametrize("n", RANK_N)
def test_truncation_rank_direct(lib, oracle_mod, n, case):
    w = graded_spectrum(n)
    assert np.all(np.diff(w) > 0) and (n < 10 or w[0] < 0)
    rule, thr = RANK_CASES[case]
    S_ref = np.sqrt(np.maximum(w, 1e-12))[::-1].copy()
    k_ref = oracle_mod.truncation_rank(S_ref, thr, rule)
    # the kernel adds sequentially, numpy pairwise: only a threshold the
    # oracle's own rank does not hinge on is a fair input
    for f in (1 - 1e-6, 1 + 1e-6):
        assert oracle_mod.truncation_rank(S_ref, thr * f, rule) == k_ref, "knife-edge input"
    dw = dev(w)
    S = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    kd = torch.full((3,), -77, dtype=torch.int32, device=DEV)
    lib.call("tg_truncation_rank", lib.stream(), lib.ptr(dw), n, thr, lib.RULES[rule], lib.ptr(S),
             ctypes.c_void_p(kd.data_ptr() + 4))
    S = S.cpu().numpy()
    kd = kd.cpu().numpy()
    print(f"tg_truncation_rank n={n} {case}: k={kd[1]} (oracle {k_ref})")
    assert bits_equal(S[:n], S_ref) and S[n] == SENTINEL
    assert kd[0] == -77 and kd[2] == -77
    assert kd[1] == k_ref
    if case in ("energy", "mean_trimmed") and n >= 33:
        assert 1 <= k_ref < n  # the rule does cut this spectrum
    if case in ("energy-all", "none"):
        assert k_ref == n


# ---------------------------------------------------------------------------
# tg_group_params
# ---------------------------------------------------------------------------
def group_params_input(m, n, g, seed):
    """Random W with the rows / groups where find_params can go wrong: all
    equal, all positive, all negative, range below the 1e-5 clamp, one huge
    outlier, all +0, all -0, signed zeros among other values."""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((m, n)) * 0.05).astype(np.float32)
    gg = n if g <= 0 else g
    G = n // gg
    patterns = [
        lambda k: np.full(k, 0.3),
        lambda k: np.abs(rng.standard_normal(k)) + 0.01,
        lambda k: -np.abs(rng.standard_normal(k)) - 0.01,
        lambda k: 1.0 + 4e-6 * rng.random(k),
        lambda k: np.where(np.arange(k) == k // 2, 1e20, rng.standard_normal(k)),
        lambda k: np.zeros(k),
        lambda k: -np.zeros(k),
        lambda k: np.resize(np.array([0.0, -0.0, 0.5, -0.25]), k),
    ]
    for i, pat in enumerate(patterns):
        r, gi = (i // G) % m, i % G
        W[r, gi * gg:(gi + 1) * gg] = pat(gg).astype(np.float32)
    return W


@pytest.mark.parametrize("m,n,g,layout", [(37, 330, -1, "C"), (37, 330, 110, "B"), (5, 96, 32, "A"),
                                          (3, 64, 1, "C")])
def test_group_params_direct(lib, oracle_mod, m, n, g, layout):
    W = group_params_input(m, n, g, m + n)
    G = n // (n if g <= 0 else g)
    pW, bW, ldw, lead = lay(W, layout)
    for bits in (2, 3, 4, 8):
        for sym in (False, True):
            s_ref, z_ref = oracle_mod.find_params(W, bits, g, sym)
            out = torch.full((2, m * G + 1), SENTINEL, dtype=torch.float32, device=DEV)
            lib.call("tg_group_params", lib.stream(), pW, m, n, ldw, g, bits, int(sym),
                     lib.ptr(out[0]), lib.ptr(out[1]))
            o = out.cpu().numpy()
            tag = f"m={m} n={n} g={g} bits={bits} sym={sym}"
            assert bits_equal(o[0, :-1].reshape(m, G), s_ref), tag
            assert bits_equal(o[1, :-1].reshape(m, G), z_ref), tag
            assert o[0, -1] == SENTINEL and o[1, -1] == SENTINEL, tag
    assert bits_equal(logical(bW, W.shape, ldw, lead), W) and outside_intact(bW, W.shape, ldw, lead)


# ---------------------------------------------------------------------------
# tg_process_block
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 31, 32, 33, 100])
def test_process_block_padded(lib, oracle_mod, B):
    """Six different leading dimensions, every operand one element into its
    allocation."""
    m, minq, maxq = 37, 0, 15
    rng = np.random.default_rng(B)
    w = (rng.standard_normal((m, B)) * 0.05).astype(np.float32)
    s = (0.005 + 0.01 * rng.random((m, B))).astype(np.float32)
    z = rng.integers(0, 16, (m, B)).astype(np.float32)
    R = np.triu(rng.standard_normal((B, B)) * 0.02)
    R[np.arange(B), np.arange(B)] = 1.0 + np.abs(rng.standard_normal(B))
    R = R.astype(np.float32)
    q_ref, e_ref = oracle_mod.process_block(w, s, z, R, minq, maxq)
    ldw, lds, ldz, ldr, ldq, lde = B + 1, B + 2, B + 3, B + 5, B + 7, B + 4
    pw, bw = padded(w, ldw, 1)
    ps, bs = padded(s, lds, 1)
    pz, bz = padded(z, ldz, 1)
    pR, bR = padded(R, ldr, 1)
    pq, bq = padded(np.zeros((m, B), np.float32), ldq, 1)
    pe, be = padded(np.zeros((m, B), np.float32), lde, 1)
    ws = lib.workspace(lib.lib.tg_process_block_workspace_size(B), DEV)
    lib.call("tg_process_block", lib.stream(), pw, ldw, ps, lds, pz, ldz, pR, ldr, m, B, minq, maxq,
             pq, ldq, pe, lde, lib.ptr(ws), ws.numel())
    assert bits_equal(logical(bq, (m, B), ldq, 1), q_ref)
    assert bits_equal(logical(be, (m, B), lde, 1), e_ref)
    assert outside_intact(bq, (m, B), ldq, 1) and outside_intact(be, (m, B), lde, 1)
    for buf, a, ld in ((bw, w, ldw), (bs, s, lds), (bz, z, ldz), (bR, R, ldr)):  # inputs unchanged
        assert bits_equal(logical(buf, a.shape, ld, 1), a) and outside_intact(buf, a.shape, ld, 1)


# ---------------------------------------------------------------------------
# tg_pack_codes / tg_pack_zeros
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["random", "max"])
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("bits", [2, 3, 4, 8])
def test_pack_direct(lib, oracle_mod, bits, sym, fill):
    m, n, G = 32, 96, 3
    rng = np.random.default_rng(bits)
    off = oracle_mod.code_offset(bits, sym)
    top = 2 ** bits - 1
    if fill == "max":
        codes_u = np.full((m, n), top, dtype=np.uint8)
        zero_u = np.full((m, G), top)
    else:
        codes_u = rng.integers(0, top + 1, (m, n)).astype(np.uint8)
        zero_u = rng.integers(off, top + 1, (m, G))
        assert codes_u.max() == top and codes_u.min() == 0
    zero = (zero_u - off).astype(np.float32)  # stored zero = zero + offset
    qw_ref, qz_ref, _ = oracle_mod.pack_weights(codes_u.astype(np.int64) - off,
                                                np.ones((m, G), np.float32), zero, bits, sym)
    nw, nz = n * bits // 32, m * bits // 32
    qw = torch.full((nw * m + 1,), 0x55555555, dtype=torch.int32, device=DEV)
    qz = torch.full((G * nz + 1,), 0x55555555, dtype=torch.int32, device=DEV)
    dc, dz = dev(codes_u), dev(zero)
    lib.call("tg_pack_codes", lib.stream(), lib.ptr(dc), m, n, bits, lib.ptr(qw))
    lib.call("tg_pack_zeros", lib.stream(), lib.ptr(dz), m, G, bits, int(sym), lib.ptr(qz))
    qw, qz = qw.cpu().numpy(), qz.cpu().numpy()
    assert qw[-1] == 0x55555555 and qz[-1] == 0x55555555
    qw, qz = qw[:-1].reshape(nw, m), qz[:-1].reshape(G, nz)
    assert np.array_equal(qw, qw_ref)
    assert np.array_equal(qz, qz_ref)
    assert np.array_equal(oracle_mod.unpack_rows_bitstream(qw, bits, n).T, codes_u)
    assert np.array_equal(oracle_mod.unpack_rows_bitstream(np.ascontiguousarray(qz.T), bits, m),
                          zero_u)


# ---------------------------------------------------------------------------
# tg_scale_f64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 255, 257, 100003])
def test_scale_f64_direct(lib, count):
    rng = np.random.default_rng(count)
    H = rng.standard_normal(count) * np.logspace(-8, 8, count)
    dH = dev(H)

    def scale(inv_n, alias=False):
        src = dH.clone()
        out = src if alias else torch.full((count + 1,), SENTINEL, dtype=torch.float64, device=DEV)
        lib.call("tg_scale_f64", lib.stream(), lib.ptr(src), count, inv_n, lib.ptr(out))
        o = out.cpu().numpy()
        if not alias:
            assert o[count] == SENTINEL
            assert bits_equal(src.cpu().numpy(), H)  # the input is left alone
        return o[:count]

    inv = 1.0 / 7.0
    assert bits_equal(scale(inv), H * inv)
    for div in (3.0, 800.0):
        exact = H / div
        if count > 1:  # multiplying by the rounded reciprocal is not the same operation
            assert not bits_equal(H * (1.0 / div), exact)
        assert bits_equal(scale(-div), exact)
    assert bits_equal(scale(-800.0, alias=True), H / 800.0)
    assert bits_equal(scale(inv, alias=True), H * inv)
