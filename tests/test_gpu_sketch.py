"""GPU: sketch mode -- the Omega generator, the fused sketch GEMM (bit for bit
the fmaf chain of include/truncgptq.h), Sketcher, process_sketch against the
reference's outputs (tests/golden/k_*), and quantize_model(mode="svd")."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden_names, load_golden

sys.path.insert(0, GOLDEN)
from make_sketch_golden import load_sketch_golden, sketch_golden_names  # noqa: E402
from test_sketch_host import omega_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def dev_omega(seed, t0, rank, T):
    from gptq_svd_amd import _lib
    Om = torch.empty((rank, T), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.call("tg_sketch_omega", _lib.stream(), seed, t0, rank, T, _lib.ptr(Om), T)
    return Om


def accum(X, seed, t0, Y, rank, n):
    """tg_sketch_accum on the leading rank x n block of Y (any row stride)."""
    from gptq_svd_amd import _lib
    with torch.cuda.device(DEV):
        _lib.call("tg_sketch_accum", _lib.stream(), _lib.ptr(X), _lib.DTYPES[X.dtype], X.shape[0],
                  n, X.stride(0), seed, t0, _lib.ptr(Y), rank, Y.stride(0))


def fmaf_chain(Y0, Om, X):
    """acc = Y0; acc = fmaf(Om[:, t], X[t, :], acc) for ascending t, on the host.

    As oracle.fma_chain_matmul: the product of two floats is exact in float64
    and each step is rounded once from float64 to float32, here starting from
    Y0.  Where the float64 sum itself rounds (an fp32 X gives 48-bit products),
    it is first rounded to odd from the exact TwoSum error, so the one rounding
    to float32 is the fused one for every exponent gap, not only for the
    unit-scale inputs the tests use."""
    acc = np.asarray(Y0, dtype=np.float32).copy()
    Om = np.asarray(Om, dtype=np.float32).astype(np.float64)
    X = np.asarray(X, dtype=np.float64)
    for t in range(X.shape[0]):
        a = acc.astype(np.float64)
        p = Om[:, t:t + 1] * X[t:t + 1, :]
        s = a + p
        bb = s - a
        err = (a - (s - bb)) + (p - bb)
        bits = s.view(np.int64)
        fix = (err != 0) & ((bits & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        acc = s.astype(np.float32)
    return acc


def unit_x(T, n, ldx, dtype, gen):
    """Unit-scale X (T x n inside a T x ldx buffer) of the given torch dtype."""
    buf = torch.randn(T, ldx, generator=gen).to(dtype).to(DEV)
    return buf[:, :n]


# --------------------------------------------------------------------------
# Omega
# --------------------------------------------------------------------------
@pytest.mark.parametrize("t0", [0, 2 ** 32 - 7])
def test_omega_matches_the_restatement(t0):
    """rank 70 x 45 tokens: odd sizes (tile edges); the second t0 crosses the
    32-bit counter word.

    Tolerance, from the documented maximum errors of the device functions called
    (HIP math API, single precision: logf 1 ulp, sqrtf 1 ulp, sincospif 1 ulp)
    with eps = 2^-24, so that 1 ulp is at most 2 eps relative.  u1 and 2 u2 are
    exact in fp32, and -2 * log is exact.  Relative errors, first order:
      logf 2 eps, halved by the square root      1 eps
      sqrtf itself                                 2 eps
      cospif / sinpif of the exact argument        2 eps
      the final product                            1 eps
    in all 6 eps = 6 * 2^-24 of |omega|.  The absolute term 1e-12 covers the
    second-order terms (36 eps^2 |omega| < 8e-13 for |omega| < 6) and the
    float64 restatement's own error (2 pi u2 is rounded: ~1e-15)."""
    seed = 0x1234_5678_9ABC_DEF1
    rank, T = 70, 45
    got = dev_omega(seed, t0, rank, T).cpu().numpy().astype(np.float64)
    want = omega_ref(seed, range(rank), [t0 + t for t in range(T)])
    assert np.isfinite(got).all()
    err = np.abs(got - want)
    tol = 6 * 2.0 ** -24 * np.abs(want) + 1e-12
    print(f"t0={t0}: max err / tol = {np.max(err / tol):.3f}")
    assert np.all(err <= tol), float(np.max(err / tol))


def test_omega_depends_on_seed_and_token():
    a = dev_omega(3, 0, 64, 64)
    assert not torch.equal(a, dev_omega(4, 0, 64, 64))
    b = dev_omega(3, 5, 64, 64)
    assert not torch.equal(a, b)
    assert torch.equal(a[:, 5:], b[:, :59])      # a function of the global token index
    assert torch.equal(a[:40], dev_omega(3, 0, 40, 64))


def test_omega_moments():
    """2^20 values: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N) (five sigma
    of the sample mean and of the sample variance of a unit Gaussian)."""
    N = 1 << 20
    om = dev_omega(99, 12345, 1024, 1024).double()
    mean, var = float(om.mean()), float(om.var(unbiased=False))
    print(f"mean {mean:.3e} (bound {5 / N ** 0.5:.3e}), var - 1 {var - 1:.3e} "
          f"(bound {5 * (2 / N) ** 0.5:.3e})")
    assert abs(mean) <= 5 / N ** 0.5
    assert abs(var - 1.0) <= 5 * (2.0 / N) ** 0.5


# --------------------------------------------------------------------------
# fused GEMM, bit-exact
# --------------------------------------------------------------------------
@pytest.mark.parametrize("rank", [32, 70, 200])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_accum_is_the_fmaf_chain(rank, dt):
    seed = 1000 + rank
    gen = torch.Generator().manual_seed(rank)
    for T in (1, 2, 37, 300):
        Om = dev_omega(seed, 17, rank, T).cpu().numpy()
        for n in (32, 72, 264):
            ldx, ldy = n + 3, n + 5
            X = unit_x(T, n, ldx, TORCH[dt], gen)
            Y0 = torch.randn(rank + 2, ldy, generator=gen)          # non-zero start, guard rows
            Y = Y0.to(DEV)
            accum(X, seed, 17, Y, rank, n)
            got = Y.cpu().numpy()
            want = fmaf_chain(Y0[:rank, :n].numpy(), Om, X.float().cpu().numpy())
            assert np.array_equal(got[:rank, :n], want), (T, n, int(np.sum(got[:rank, :n] != want)))
            # columns >= n of the rows, and the rows past the rank, are untouched
            assert np.array_equal(got[:, n:], Y0[:, n:].numpy()), (T, n)
            assert np.array_equal(got[rank:], Y0[rank:].numpy()), (T, n)


@pytest.mark.parametrize("rank,n,T", [(300, 520, 1100), (530, 130, 70)])
def test_accum_many_tiles_and_k_steps(rank, n, T):
    """Five column tiles of 128 and 35 K tiles of 32 tokens; then two row tiles
    of 512 (with an idle wave in the second), two column tiles, three K tiles."""
    seed = 77
    gen = torch.Generator().manual_seed(5)
    X = unit_x(T, n, n + 8, torch.float16, gen)
    Y0 = torch.randn(rank, n + 1, generator=gen)
    Y = Y0.to(DEV)
    accum(X, seed, 3, Y, rank, n)
    Om = dev_omega(seed, 3, rank, T).cpu().numpy()
    want = fmaf_chain(Y0[:, :n].numpy(), Om, X.float().cpu().numpy())
    got = Y.cpu().numpy()
    assert np.array_equal(got[:, :n], want), int(np.sum(got[:, :n] != want))
    assert np.array_equal(got[:, n:], Y0[:, n:].numpy())


def test_split_and_rank_invariance():
    n, T, seed = 264, 300, 5
    gen = torch.Generator().manual_seed(9)
    X = unit_x(T, n, n, torch.float16, gen)
    Y0 = torch.randn(200, n, generator=gen)
    one = Y0.to(DEV)
    accum(X, seed, 40, one, 200, n)
    again = Y0.to(DEV)
    accum(X, seed, 40, again, 200, n)
    assert torch.equal(one, again)
    parts = Y0.to(DEV)
    t = 0
    for cnt in (128, 1, 171):
        accum(X[t:t + cnt], seed, 40 + t, parts, 200, n)
        t += cnt
    assert torch.equal(one, parts)
    small = Y0[:70].to(DEV)
    accum(X, seed, 40, small, 70, n)
    assert torch.equal(one[:70], small)


# --------------------------------------------------------------------------
# process_sketch against the reference's outputs
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sketch_golden_names())
def test_process_sketch_matches_reference(name):
    import gptq_svd_amd.gptq_utils as g
    d = load_sketch_golden(name)
    R, perm = g.process_sketch(torch.from_numpy(d["Y"]).to(DEV), threshold=float(d["eps"]),
                               threshold_method=str(d["method"]))
    assert R.dtype == torch.float64 and perm.dtype == torch.int64
    assert R.shape == (int(d["k"]), d["Y"].shape[1])
    assert np.array_equal(perm.cpu().numpy(), d["perm"])
    err = np.linalg.norm(R.cpu().numpy() - d["R"]) / np.linalg.norm(d["R"])
    print(f"{name}: k={R.shape[0]} |R - R_ref|/|R_ref| = {err:.2e}")
    assert err < 1e-8, err


def test_the_goldens_cover_the_cases():
    assert len(sketch_golden_names()) >= 3


def test_process_sketch_unknown_method():
    import gptq_svd_amd.gptq_utils as g
    with pytest.raises(ValueError):
        g.process_sketch(torch.zeros(8, 4, device=DEV), threshold_method="bogus")


# --------------------------------------------------------------------------
# Sketcher
# --------------------------------------------------------------------------
def test_sketcher_hook_and_scaling():
    import gptq_svd_amd.gptq_utils as g
    lin = torch.nn.Linear(72, 8)
    sk = g.Sketcher(lin, 100, device=DEV, seed=11)
    assert sk.rank == 100 and sk.in_features == 72 and sk.n_samples == 0
    assert sk.Y.shape == (100, 72) and sk.Y.dtype == torch.float32
    assert sk.get_scaled_sketch() == (None, None, 0)
    x = torch.randn(3, 7, 72, generator=torch.Generator().manual_seed(1)).half().to(DEV)
    sk.hook_fn(lin, (x,), None)
    assert sk.n_samples == 21
    sk.hook_fn(lin, (x[:0],), None)                      # an empty batch is ignored
    assert sk.n_samples == 21
    sk.hook_fn(lin, (x.reshape(21, 72)[:5].double(),), None)   # other dtypes: cast to fp32
    assert sk.n_samples == 26
    raw = sk.Y.clone()
    # the same tokens through the bare kernel
    Y = torch.zeros(100, 72, device=DEV)
    accum(x.reshape(21, 72), 11, 0, Y, 100, 72)
    accum(x.reshape(21, 72)[:5].float(), 11, 21, Y, 100, 72)
    assert torch.equal(raw, Y)
    out = sk.get_scaled_sketch()
    assert out is sk.Y
    want = raw.double() / np.sqrt(26 * 100)
    assert torch.allclose(out.double(), want, rtol=2.0 ** -22, atol=0)   # two fp32 roundings


def test_sketcher_seeding():
    import gptq_svd_amd.gptq_utils as g
    lin = torch.nn.Linear(40, 8)
    x = torch.randn(50, 40, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).to(DEV)

    def run(seed):
        sk = g.Sketcher(lin, 64, device=DEV, seed=seed)
        sk.add_batch(x)
        return sk

    assert torch.equal(run(5).Y, run(5).Y)
    assert not torch.equal(run(5).Y, run(6).Y)
    runs = []
    for _ in range(2):
        torch.manual_seed(1234)
        a, b = run(None), run(None)
        assert a.seed != b.seed and 0 <= a.seed < 2 ** 63
        runs.append((a.Y, b.Y))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][0], runs[0][1])


def test_sketch_is_unbiased():
    """Y_s^T Y_s estimates H = X^T X / N.  With Y_s = Omega X / sqrt(N rank) and
    Gaussian Omega, Y_s^T Y_s = (1 / rank) sum_r z_r z_r^T with z_r ~ N(0, H)
    independent: a Wishart matrix of `rank` degrees of freedom over rank.  Its
    entry (i, j) has variance (H_ij^2 + H_ii H_jj) / rank, so
      E ||Y_s^T Y_s - H||_F^2 = (||H||_F^2 + tr(H)^2) / rank,
    i.e. one standard deviation of the relative Frobenius error is
      rho = sqrt((1 + tr(H)^2 / ||H||_F^2) / rank).
    The bound is 6 rho.  At rank = 8 n = 512 on the ar1 input rho is about
    0.12, so the bound is about 0.74: the reference's commented-out scale
    sqrt(N rank / 2) (Y_s^T Y_s = 2 H, relative error 1.0) fails it, and so do
    rows that share their omegas (error ~ rho sqrt(rank / distinct rows))."""
    import gptq_svd_amd.gptq_utils as g
    from synth import make_x
    n, N, rank = 64, 4096, 512
    X = make_x("ar1", N, n, torch.Generator().manual_seed(21))
    sk = g.Sketcher(torch.nn.Linear(n, 8), rank, device=DEV, seed=2024)
    for j in range(0, N, 1000):
        sk.add_batch(X[j:j + 1000].to(DEV))
    Ys = sk.get_scaled_sketch().double().cpu().numpy()
    Xd = X.double().numpy()
    H = Xd.T @ Xd / N
    rho = np.sqrt((1.0 + np.trace(H) ** 2 / np.linalg.norm(H) ** 2) / rank)
    err = np.linalg.norm(Ys.T @ Ys - H) / np.linalg.norm(H)
    print(f"relative error {err:.4f}, rho {rho:.4f}, bound {6 * rho:.4f}")
    assert err <= 6 * rho


# --------------------------------------------------------------------------
# harness
# --------------------------------------------------------------------------
def tiny_qwen3():
    """The tiny random Qwen3 of the harness goldens (config, initial weights and
    calibration ids are data in tests/golden/h_*.npz)."""
    from transformers import Qwen3Config, Qwen3ForCausalLM
    d = load_golden(golden_names("h_")[0])
    cfg = Qwen3Config(**json.loads(str(d["config"])))
    cfg._attn_implementation = "eager"
    m = Qwen3ForCausalLM(cfg).float().eval()
    m.load_state_dict({k[len("init/"):]: torch.from_numpy(d[k]) for k in d
                       if k.startswith("init/")})
    return m.to(DEV), [torch.from_numpy(r[None]) for r in d["ids"]]


KW = dict(mode="svd", sketch_ratio=4.0, sketch_seed=7, w_bits=4, group_size=128, sym=False,
          eps=1e-2, threshold_method="mean_trimmed", batch_size=3, device=DEV, pack=True)


@pytest.fixture(scope="module")
def svd_runs():
    from gptq_svd_amd import harness
    out = {}
    for staged in (True, False):
        model, ids = tiny_qwen3()
        assert harness._staged_layer(harness.get_layers(model)[0])
        res = harness.quantize_model(model, ids, staged=staged, **KW)
        out[staged] = (model, res)
    return out


def test_svd_mode_staged_matches_generic(svd_runs):
    (m1, r1), (m2, r2) = svd_runs[True], svd_runs[False]
    assert [s["rank"] for s in r1["layer_stats"]] == [s["rank"] for s in r2["layer_stats"]]
    assert len(r1["layer_stats"]) == 14 and all(isinstance(s["rank"], int) and s["rank"] >= 1
                                                for s in r1["layer_stats"])
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    changed = 0
    orig = tiny_qwen3()[0].state_dict()
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
        changed += int(not torch.equal(sd1[k], orig[k]))
    assert changed == 14                                     # every sequenced linear was quantised


def test_svd_mode_first_group_by_hand(svd_runs):
    """Layer 0's q/k/v: the harness equals Sketcher(seed=7) -> process_sketch ->
    gptq_fwrd on the same inputs, bit for bit."""
    import gptq_svd_amd.gptq_utils as g
    from gptq_svd_amd import harness
    model, ids = tiny_qwen3()
    layer = harness.get_layers(model)[0]
    attn = layer.self_attn
    sk = g.Sketcher(attn.q_proj, int(attn.q_proj.in_features * 4.0), device=DEV, seed=7)
    with torch.no_grad():
        inps, _ = harness.capture_initial_inputs(model, ids, device=DEV, batch_size=3)
        for j in range(0, inps.shape[0], 3):
            sk.hook_fn(attn.q_proj, (layer.input_layernorm(inps[j:j + 3]),), None)
    assert sk.n_samples == inps.shape[0] * inps.shape[1]
    R, perm = g.process_sketch(sk.get_scaled_sketch(), threshold=1e-2,
                               threshold_method="mean_trimmed")
    got = svd_runs[True][0].state_dict()
    stats = {s["name"]: s["rank"] for s in svd_runs[True][1]["layer_stats"]}
    for name in ("q_proj", "k_proj", "v_proj"):
        W = getattr(attn, name).weight.data.float()
        Wq, k = g.gptq_fwrd(W, R, g.Quantizer(4, 128, False), perm, block_size=1024,
                            use_triton=True)
        assert torch.equal(Wq, got[f"model.layers.0.self_attn.{name}.weight"]), name
        assert stats[f"layer_0.self_attn.{name}"] == k == R.shape[0]


def test_svd_mode_packed_codes_decode(svd_runs, oracle_mod):
    model, res = svd_runs[True]
    sd = model.state_dict()
    assert len(res["packed"]) == 14
    for name, t in res["packed"].items():
        W = sd[name + ".weight"].float().cpu().numpy()
        m, n = W.shape
        codes = oracle_mod.unpack_rows_bitstream(t["qweight"].cpu().numpy(), 4, n).T
        zeros = oracle_mod.unpack_rows_bitstream(t["qzeros"].cpu().numpy().T, 4, m)
        scales = t["scales"].float().cpu().numpy()               # (G, m)
        gi = np.arange(n) // 128
        deq = (codes.astype(np.float32) - zeros[:, gi].astype(np.float32)) * scales.T[:, gi]
        assert np.array_equal(deq, W), name


def test_svd_mode_records_the_run(tmp_path):
    """results.json carries the ratio and the seed the run used (not the
    reference's defaults), and the ratio sets the sketch rank."""
    from gptq_svd_amd import harness
    model, ids = tiny_qwen3()
    kw = dict(KW, sketch_ratio=2.0, sketch_seed=9)
    ranks = []
    real = harness.Sketcher

    class Spy(real):
        def __init__(self, layer, rank, device="cuda", seed=None):
            ranks.append((layer.in_features, rank, seed))
            super().__init__(layer, rank, device=device, seed=seed)

    harness.Sketcher = Spy
    try:
        res = harness.quantize_model(model, ids, save_path=str(tmp_path), **kw)
    finally:
        harness.Sketcher = real
    assert len(ranks) == 8 and all(r == 2 * n and s == 9 for n, r, s in ranks)
    rec = json.load(open(os.path.join(str(tmp_path), "results.json")))
    assert rec["config"]["mode"] == "svd"
    assert rec["config"]["sketch_ratio"] == 2.0 and rec["config"]["sketch_seed"] == 9
    assert [s["rank"] for s in rec["layer_stats"]] == [s["rank"] for s in res["layer_stats"]]


@pytest.mark.parametrize("how", ["full_pass", "offload"])
def test_svd_mode_full_pass_and_offload(svd_runs, how):
    """early_stop=False (every calibration pass runs the whole layer, the hook
    only accumulates) gives the weights of the early-stopping runs bit for
    bit.  offload=True starts from a model on the CPU and moves one layer at a
    time: the embedding lookup is exact, so layer 0's q/k/v (whose inputs do not
    pass through the rotary tables, computed on the CPU in this mode) are
    bit-identical too, and every sequenced linear is quantised."""
    from gptq_svd_amd import harness
    model, ids = tiny_qwen3()
    ref = svd_runs[False][0].state_dict()
    if how == "full_pass":
        res = harness.quantize_model(model, ids, early_stop=False, **KW)
        same = list(ref)
    else:
        model = model.cpu()
        res = harness.quantize_model(model, ids, offload=True, **KW)
        assert next(model.parameters()).device.type == "cpu"
        same = [f"model.layers.0.self_attn.{n}.weight" for n in ("q_proj", "k_proj", "v_proj")]
    assert len(res["layer_stats"]) == 14 and len(res["packed"]) == 14
    sd = model.state_dict()
    for k in same:
        assert torch.equal(sd[k].cpu(), ref[k].cpu()), k
    orig = tiny_qwen3()[0].state_dict()
    assert sum(int(not torch.equal(sd[k].cpu(), orig[k].cpu())) for k in sd) == 14


def test_svd_quality_beats_round_to_nearest():
    """ar1-correlated calibration X, n=256, m=96, 4-bit g128, 2048 tokens, sketch
    ratio 4: the proxy error ||(W - Wq) X^T||_F of sketch mode is below
    round-to-nearest's on the same grid (the CPU oracle gave 0.51 x RTN)."""
    import gptq_svd_amd.gptq_utils as g
    from synth import make_x
    n, m, N = 256, 96, 2048
    gen = torch.Generator().manual_seed(31)
    X = make_x("ar1", N, n, gen)
    W = (torch.randn(m, n, generator=gen) * 0.05).to(DEV)
    sk = g.Sketcher(torch.nn.Linear(n, m), 4 * n, device=DEV, seed=1)
    sk.add_batch(X.to(DEV))
    R, perm = g.process_sketch(sk.get_scaled_sketch(), threshold=1e-2,
                               threshold_method="mean_trimmed")
    q = g.Quantizer(4, 128, False)
    Wq, _ = g.gptq_fwrd(W, R, q, perm, block_size=1024, use_triton=True)
    s, z = q.get_expanded_params(m, n)
    rtn = (torch.clamp(torch.round(W / s + z), q.min_q, q.max_q) - z) * s
    Xd = X.double().to(DEV)
    e_svd = float(torch.linalg.norm((W - Wq).double() @ Xd.T))
    e_rtn = float(torch.linalg.norm((W - rtn).double() @ Xd.T))
    print(f"svd {e_svd:.4f}, rtn {e_rtn:.4f}, ratio {e_svd / e_rtn:.3f}")
    assert e_svd < e_rtn
