"""GPU: the whole solver on Hessians with dead (identically zero) and duplicated
input channels -- inputs and host references in tests/degenerate_ref.py, which
tests/test_degenerate_ref.py proves on the CPU to meet every bar used here.

  a  accumulation: H's dead rows / columns exactly 0, H == H.T, 1e-14 to the
     float64 product (test_gpu_syrk.py); the sketch's dead columns exactly 0
     and duplicated columns bit-equal (one fmaf chain per entry);
  b  eigensolver, k = n: the bars of test_gpu_solver.py::test_eigh with the
     residual bar for exactly repeated eigenvalues (the null space);
  c  pivot stage alone, nc = 0, k = structural rank: perm identical to
     test_complement_math.pivoted_cholesky, R_x <= 1e-10 (test_gpu_pivot.py);
  d  truncated_spectral_factor on both spectral paths: U and R_x within 1e-8
     (test_process_hessian_alt_golden) of the reference's factors for the
     GPU's own perm (the choice inside a duplicated pair is arbitrary);
  e  quantize: codes given U bit-exact (test_gpu_small_stages.py), dead
     columns are round-to-nearest, the solve beats round-to-nearest;
  f  the harness on a tiny OPT whose fc2 reads 16 dead post-ReLU features.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import degenerate_ref as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


@pytest.fixture(scope="module")
def g():
    import gptq_svd_amd.gptq_utils as g
    return g


@pytest.fixture(scope="module")
def lib():
    from gptq_svd_amd import _lib
    return _lib


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)          # a copy: the inputs are read-only
    return t if dtype is None else t.to(dtype)


def bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(u), b.view(u))


@contextlib.contextmanager
def env(**kw):
    """Set (value) or unset (None) environment variables for one library call."""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def gpu_hessian(g, X, dtype=torch.float16):
    acc = g.HessianAccumulator(X.shape[1], DEV)
    acc.add_batch(dev(X, dtype))
    return acc, acc.get_hessian()


# ---------------------------------------------------------------------------
# a. accumulation
# ---------------------------------------------------------------------------
ACC_SHAPE = (300, 256, 9, 6, 3)   # N, n, dead, pairs, seed


@pytest.mark.parametrize("dt,lds64", [("f16", "0"), ("f16", "1"), ("bf16", "0"), ("bf16", "1"),
                                      ("f32", None)])
def test_accumulate(g, monkeypatch, dt, lds64):
    if lds64 is not None:
        monkeypatch.setenv("TG_SYRK_LDS64", lds64)
    X, dead, pairs = D.degenerate_x(*ACC_SHAPE)
    Xt = torch.from_numpy(X).to(TORCH[dt])               # bf16 rounds; zeros and pairs survive
    acc = g.HessianAccumulator(X.shape[1], DEV)
    acc.add_batch(Xt.to(DEV))
    assert acc.n_samples == X.shape[0]
    H = acc.get_hessian().cpu().numpy()
    X64 = Xt.double().numpy()
    ref = X64.T @ X64 / X.shape[0]
    err = D.rel(H, ref)
    print(f"[a] syrk {dt} lds64={lds64}: rel {err:.2e} (bar 1e-14)")
    assert not H[dead].any() and not H[:, dead].any(), "dead rows / columns must be exactly 0"
    assert np.array_equal(H, H.T)
    assert err <= 1e-14


def test_sketch_accumulate(lib):
    X, dead, pairs = D.degenerate_x(*ACC_SHAPE)
    T, n = X.shape
    rank = 70
    Xd = dev(X)
    Y = torch.zeros((rank, n), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        lib.call("tg_sketch_accum", lib.stream(), lib.ptr(Xd), lib.DTYPES[Xd.dtype], T, n,
                 Xd.stride(0), 77, 0, lib.ptr(Y), rank, Y.stride(0))
    Y = Y.cpu().numpy()
    assert np.isfinite(Y).all() and Y.any()
    assert not Y[:, dead].any(), "dead columns of the sketch must be exactly 0"
    for a, b in pairs:
        assert bits_equal(Y[:, a], Y[:, b]), (a, b)


# ---------------------------------------------------------------------------
# b. eigensolver
# ---------------------------------------------------------------------------
def run_eigh(lib, H):
    n = H.shape[0]
    A = dev(H).clone()
    ws = lib.workspace(lib.lib.tg_eigh_workspace_size(n), DEV)
    w = torch.empty(n, dtype=torch.float64, device=DEV)
    lib.call("tg_eigh_values", lib.stream(), lib.ptr(A), n, n, lib.ptr(w), lib.ptr(ws), ws.numel())
    Vh = torch.empty((n, n), dtype=torch.float64, device=DEV)
    lib.call("tg_eigh_vectors", lib.stream(), n, lib.ptr(w), n, lib.ptr(Vh), n, lib.ptr(ws),
             ws.numel())
    torch.cuda.synchronize()
    return w.cpu().numpy(), Vh.cpu().numpy()


def eigh_and_check(lib, name, tag):
    H = D.EIGH_CASES[name]
    w, Vh = run_eigh(lib, H)
    fig = D.check_eigh(name, H, w, Vh)
    print(f"[b] eigh {name} {tag}: eig {fig['eig']:.2e} resid {fig['resid']:.2e} "
          f"orth {fig['orth']:.2e}")
    return w


@pytest.mark.parametrize("name", D.EIGH_NAMES)
def test_eigh_degenerate(lib, name):
    eigh_and_check(lib, name, "default")


PANEL_MODES = {"default": {}, "fallback": {"TG_PQR_FALLBACK": "1"}, "tsqr": {"TG_SB_TSQR": "1"}}


@pytest.mark.parametrize("mode", list(PANEL_MODES))
@pytest.mark.parametrize("name", ["both200", "both600"])
def test_eigh_degenerate_panel_modes(lib, monkeypatch, name, mode):
    for k, v in PANEL_MODES[mode].items():
        monkeypatch.setenv(k, v)
    eigh_and_check(lib, name, mode)


@pytest.mark.parametrize("var,val", [("TG_EIGH_TWOSTAGE", "0"), ("TG_BISECT_CHUNK", "1")])
def test_eigh_degenerate_switches(lib, monkeypatch, var, val):
    monkeypatch.setenv(var, val)
    eigh_and_check(lib, "both200", f"{var}={val}")


def test_eigh_degenerate_deterministic(lib):
    H = D.EIGH_CASES["both600"]
    w1, _ = run_eigh(lib, H)
    w2, _ = run_eigh(lib, H)
    assert bits_equal(w1, w2)


# ---------------------------------------------------------------------------
# c. pivot stage alone
# ---------------------------------------------------------------------------
def pivot_solve(lib, H, k):
    n = H.shape[0]
    Hd = dev(H)
    perm = torch.empty(n, dtype=torch.int64, device=DEV)
    Rx = torch.empty((k, n), dtype=torch.float64, device=DEV)
    ws = lib.workspace(lib.lib.tg_pivot_workspace_size(n, k), torch.device(DEV))
    lib.call("tg_pivoted_factor_complement", lib.stream(), lib.ptr(Hd), n, None, n, None, 0, n, k,
             lib.ptr(perm), lib.ptr(Rx), n, lib.ptr(ws), ws.numel())
    torch.cuda.synchronize()
    return perm.cpu().numpy(), Rx.cpu().numpy()


PIVOT_RUNS = [(c, None) for c in D.PIVOT_CASES] + [(c, "256") for c in D.PIVOT_CASES[:2]]


@pytest.mark.parametrize("case,level", PIVOT_RUNS,
                         ids=["n%d-d%d-p%d-%s" % (c + (lv or "adaptive",)) for c, lv in PIVOT_RUNS])
def test_pivot_stage(lib, monkeypatch, case, level):
    if level is None:
        monkeypatch.delenv("TG_PIV_LEVEL", raising=False)
    else:
        monkeypatch.setenv("TG_PIV_LEVEL", level)
    H, k, order, Rx_ref, dead, pairs = D.pivot_case(case)
    p, Rx = pivot_solve(lib, H, k)
    assert np.isfinite(Rx).all()
    assert np.array_equal(p[:k], order[:k]), f"first mismatch at {np.argmax(p[:k] != order[:k])}"
    assert np.array_equal(p, order), "dgeqp3 tail order differs"
    err = D.rel(Rx, Rx_ref)
    print(f"[c] pivot {case} level={level}: R_x rel {err:.2e} (bar 1e-10)")
    assert err <= 1e-10


# ---------------------------------------------------------------------------
# d. the whole factor
# ---------------------------------------------------------------------------
_FACTORS = {}


def factor(g, case, path):
    """truncated_spectral_factor on the library's own H, once per (inputs, rule,
    path); path None = the default choice.  -> dict of host arrays + U, perm on
    the device."""
    n, rule, thr = case[0], case[7], case[8]
    key = (n, rule, thr, path)
    if key not in _FACTORS:
        X, dead, pairs, W = D.pipe_inputs(case)
        _, H = gpu_hessian(g, X)
        with env(TG_SPECTRAL_PATH=path):
            U, R_x, perm, S, k = g.truncated_spectral_factor(H, thr, rule)
            last_path = g.truncated_spectral_factor.last_path
            ufac = g.truncated_spectral_factor.last_ufactor
        _FACTORS[key] = dict(H=H.cpu().numpy(), Hd=H, U=U, R_x=R_x, perm=perm, k=k,
                             S=S.cpu().numpy(), last_path=last_path, ufactor=ufac)
    return _FACTORS[key]


def check_factor(tag, M, ref, k, tol=1e-8):
    err = D.rel(M, ref)
    print(f"[d] {tag}: rel {err:.2e} (bar {tol:g})")
    assert np.isfinite(M).all(), tag
    assert err <= tol, tag
    assert np.all(np.tril(M[:, :k], -1) == 0.0), f"{tag}: strict lower triangle not 0"
    assert np.all(np.diag(M[:, :k]) > 0), tag
    return err


@pytest.mark.parametrize("path", ["kept", "complement"])
@pytest.mark.parametrize("case", D.PIPE_CASES, ids=D.PIPE_IDS)
def test_whole_factor(g, oracle_mod, case, path):
    n, rule, thr = case[0], case[7], case[8]
    X, dead, pairs, W = D.pipe_inputs(case)
    f = factor(g, case, path)
    H = f["H"]
    assert not H[dead].any() and not H[:, dead].any()
    print(f"[d] n={n} {rule} {path}: last_path {f['last_path']}, last_ufactor {f['ufactor']}")
    if path == "complement":
        # R11 is nonsingular at k = rank: a breakdown that reruns the kept path fails here
        assert f["last_path"] == ("complement", 0)
    else:
        assert f["last_path"][0] == "kept"
    ref = oracle_mod.process_hessian_alt(H, thr, rule)
    k = f["k"]
    assert k == ref.k == D.structural_rank(n, dead, pairs)
    perm = f["perm"].cpu().numpy()
    D.check_perm(perm, k, n, dead, pairs)
    s_err = D.rel(f["S"], ref.S)
    print(f"[d] n={n} {rule} {path}: S rel {s_err:.2e} (bar 1e-12)")
    assert np.isfinite(f["S"]).all() and s_err <= 1e-12
    U_ref, Rx_ref = D.factors_given_perm(H, k, perm)
    U, R_x = f["U"].cpu().numpy(), f["R_x"].cpu().numpy()
    assert U.shape == R_x.shape == (k, n)
    check_factor(f"n={n} {rule} {path} U", U, U_ref, k)
    check_factor(f"n={n} {rule} {path} R_x", R_x, Rx_ref, k)


def test_process_sketch_degenerate(g, oracle_mod):
    """The rank-512 sketch of the n = 384 X: Y has exactly zero and exactly
    repeated columns, so G = Y^T Y has the same null space as H."""
    case = D.PIPE_CASES[1]
    n = case[0]
    X, dead, pairs, W = D.pipe_inputs(case)
    sk = g.Sketcher(torch.nn.Linear(n, 8), 512, device=DEV, seed=5)
    sk.add_batch(dev(X))
    Y = sk.get_scaled_sketch()
    Yh = Y.cpu().numpy()
    assert not Yh[:, dead].any()
    for a, b in pairs:
        assert bits_equal(Yh[:, a], Yh[:, b])
    # the rank the rule must give, from LAPACK on the same sketch; not a knife-edge
    Y64 = Yh.astype(np.float64)
    G = Y64.T @ Y64
    lam = np.linalg.eigvalsh(G)[::-1]
    S = np.sqrt(np.maximum(lam, 1e-12))
    k_ref = oracle_mod.truncation_rank(S, 1e-9, "energy")
    for fac in (1 - 1e-6, 1 + 1e-6):
        assert oracle_mod.truncation_rank(S, 1e-9 * fac, "energy") == k_ref
    assert k_ref == D.structural_rank(n, dead, pairs)
    R, perm = g.process_sketch(Y, threshold=1e-9, threshold_method="energy")
    print(f"[d] process_sketch: k={R.shape[0]}, last_path "
          f"{g.truncated_spectral_factor.last_path}, last_ufactor "
          f"{g.truncated_spectral_factor.last_ufactor}")
    R, perm = R.cpu().numpy(), perm.cpu().numpy()
    assert R.shape == (k_ref, n) and np.isfinite(R).all()
    D.check_perm(perm, k_ref, n, dead, pairs)
    assert np.all(np.tril(R[:, :k_ref], -1) == 0.0) and np.all(np.diag(R[:, :k_ref]) > 0)
    err = D.rel(R, D.factors_given_perm(G, k_ref, perm)[0])
    print(f"[d] process_sketch: R vs the given-perm reference {err:.2e} (bar 1e-8)")
    assert err <= 1e-8      # the bar of test_process_sketch_matches_reference


# ---------------------------------------------------------------------------
# e. quantize
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("use_triton", [True, False], ids=["block", "loop"])
@pytest.mark.parametrize("case", D.PIPE_CASES, ids=D.PIPE_IDS)
def test_quantize(g, oracle_mod, case, use_triton):
    n, m, nd, npair, bits, group, sym, rule, thr = case
    X, dead, pairs, W = D.pipe_inputs(case)
    f = factor(g, case, None)
    k = f["k"]
    assert k > D.PIPE_BLOCK and n - k >= 12          # several blocks and a real tail
    U32 = f["U"].float().cpu().numpy()
    perm = f["perm"].cpu().numpy()
    ref, _, codes = oracle_mod.gptq_fwrd(W, U32, perm, bits, group, sym, D.PIPE_BLOCK, gemm="fma",
                                         impl="c", return_codes=True, use_triton=use_triton)
    codes = codes + oracle_mod.code_offset(bits, sym)
    q = g.Quantizer(bits, group, sym)
    Wd = dev(W)
    Wq, kk = g.gptq_fwrd(Wd, f["U"], q, f["perm"], block_size=D.PIPE_BLOCK, use_triton=use_triton)
    assert kk == k
    Wqh = Wq.cpu().numpy()
    assert bits_equal(Wqh, ref), f"{np.mean(Wqh != ref)} of elements differ"
    assert np.array_equal(q.codes.cpu().numpy().astype(np.int64), codes)
    Wrtn = D.rtn(W, bits, group, sym)
    assert bits_equal(Wqh[:, dead], Wrtn[:, dead])
    e_solve = g.log_quantization_error(Wd, Wq, f["R_x"], f["perm"])
    e_rtn = g.log_quantization_error(Wd, dev(Wrtn), f["R_x"], f["perm"])
    print(f"[e] n={n} w{bits} {'block' if use_triton else 'loop'}: prediction error "
          f"solve {e_solve:.4f}, rtn {e_rtn:.4f}")
    assert np.isfinite(e_solve) and e_solve < e_rtn


def test_quantize_mx(g):
    import mx_ref as R
    case = D.PIPE_CASES[1]
    X, dead, pairs, W = D.pipe_inputs(case)
    f = factor(g, case, None)
    U32 = f["U"].float().cpu().numpy()
    perm = f["perm"].cpu().numpy()
    want = R.gptq_fwrd_mx(W, U32, perm, D.PIPE_BLOCK, False)
    q = g.Quantizer(4, 32, weight_format="mxfp4")
    Wd = dev(W)
    Wq, kk = g.gptq_fwrd(Wd, f["U"], q, f["perm"], block_size=D.PIPE_BLOCK, use_triton=True)
    Wqh = Wq.cpu().numpy()
    assert kk == f["k"]
    assert bits_equal(Wqh, want[0]), f"{np.mean(Wqh != want[0])} of elements differ"
    assert np.array_equal(q.codes.cpu().numpy(), want[1])
    assert np.array_equal(q.scale_e8m0.cpu().numpy(), want[3])
    cast = R.rtn(W)[0]
    assert bits_equal(Wqh[:, dead], cast[:, dead])
    e_solve = g.log_quantization_error(Wd, Wq, f["R_x"], f["perm"])
    e_rtn = g.log_quantization_error(Wd, dev(cast), f["R_x"], f["perm"])
    print(f"[e] mx: prediction error solve {e_solve:.4f}, casting {e_rtn:.4f}")
    assert np.isfinite(e_solve) and e_solve < e_rtn


def test_gptq_comparator(g, oracle_mod):
    """tg_hinv_chol and the GPTQ loop on the degenerate H (actorder off): the
    damping makes the zero diagonals 0.01 mean(diag H)."""
    case = D.PIPE_CASES[1]
    n, m, nd, npair, bits, group, sym, rule, thr = case
    X, dead, pairs, W = D.pipe_inputs(case)
    f = factor(g, case, None)
    R_ref, perm_ref, rung = oracle_mod.process_hessian(f["H"], actorder=False, damp_percent=0.01)
    assert rung == 0
    R, perm = g.process_hessian(f["Hd"], actorder=False, damp_percent=0.01)
    Rh = R.cpu().numpy()
    assert np.array_equal(perm.cpu().numpy(), perm_ref)
    err = D.rel(Rh, R_ref)
    print(f"[e] hinv_chol: rel {err:.2e} (bar 1e-9)")
    assert np.isfinite(Rh).all() and err <= 1e-9
    assert np.all(np.tril(Rh, -1) == 0.0) and np.all(np.diag(Rh) > 0)
    ref, _, codes = oracle_mod.gptq_fwrd(W, Rh.astype(np.float32), perm_ref, bits, group, sym,
                                         D.PIPE_BLOCK, gemm="fma", impl="c", return_codes=True,
                                         use_triton=False)
    q = g.Quantizer(bits, group, sym)
    Wq, _ = g.gptq_fwrd(dev(W), R, q, perm, block_size=D.PIPE_BLOCK, use_triton=False)
    assert bits_equal(Wq.cpu().numpy(), ref)
    assert np.array_equal(q.codes.cpu().numpy().astype(np.int64),
                          codes + oracle_mod.code_offset(bits, sym))


# ---------------------------------------------------------------------------
# f. end to end
# ---------------------------------------------------------------------------
def dead_opt():
    """tiny_opt(11) with 16 fc1 rows zeroed and their bias at -1 in every
    decoder layer: ReLU makes those 16 fc2 inputs exactly 0."""
    from test_gpu_opt import tiny_opt
    model = tiny_opt(11)
    dead = np.sort(np.random.default_rng(5).permutation(512)[:16])
    idx = torch.from_numpy(dead)
    with torch.no_grad():
        for layer in model.model.decoder.layers:
            layer.fc1.weight[idx] = 0.0
            layer.fc1.bias[idx] = -1.0
    gen = torch.Generator().manual_seed(12)
    ids = [torch.randint(0, 256, (1, 32), generator=gen) for _ in range(8)]
    return model.to(DEV), ids, dead


@pytest.mark.parametrize("mode", ["eigh", "svd"])
def test_tiny_opt_with_dead_features(oracle_mod, mode):
    from gptq_svd_amd.harness import quantize_model
    model, ids, dead = dead_opt()
    layers = model.model.decoder.layers
    W0 = [l.fc2.weight.detach().float().cpu().numpy().copy() for l in layers]
    kw = dict(sketch_seed=7) if mode == "svd" else {}
    res = quantize_model(model, ids, mode=mode, w_bits=4, group_size=128, sym=False, eps=1e-4,
                         threshold_method="energy", batch_size=4, device=DEV, pack=True, **kw)
    for name, p in model.state_dict().items():
        assert not p.is_floating_point() or torch.isfinite(p).all(), name
    assert len(res["layer_stats"]) == 12
    for i, layer in enumerate(layers):
        got = layer.fc2.weight.detach().float().cpu().numpy()
        assert not np.array_equal(got, W0[i])
        assert bits_equal(got[:, dead], D.rtn(W0[i], 4, 128, False)[:, dead]), (mode, i)
    if mode != "eigh":
        return
    for s in res["layer_stats"]:
        if s["name"].endswith("fc2"):
            print(f"[f] {s['name']}: rank {s['rank']}")
            assert 1 <= s["rank"] <= 512 - 16
    assert len(res["packed"]) == 12
    for name_mod, t in res["packed"].items():
        W = model.get_submodule(name_mod).weight.detach().float().cpu().numpy()
        m, n = W.shape
        codes = oracle_mod.unpack_rows_bitstream(t["qweight"].cpu().numpy(), 4, n).T
        zeros = oracle_mod.unpack_rows_bitstream(t["qzeros"].cpu().numpy().T, 4, m)
        scales = t["scales"].float().cpu().numpy()
        gi = np.arange(n) // 128
        deq = (codes.astype(np.float32) - zeros[:, gi].astype(np.float32)) * scales.T[:, gi]
        assert np.array_equal(deq, W), name_mod
