"""CPU: the host restatement of the low-rank correction (tests/lrc_ref.py) meets,
on exactly the inputs test_gpu_lrc.py uses, bars 100x tighter than the GPU test
asks of the library; and the Python argument errors that need no GPU.

  - the three routes of the library (E H E^T; M M^T; M^T M with Q = M P mu^-1/2)
    agree with the SVD of E H^(1/2) in A B to 1e-10 ||E||_F (GPU bar: 1e-8);
  - Eckart-Young: tr((E - AB) H (E - AB)^T) equals the tail sum of the spectrum
    to 1e-10 relative (GPU bar: 1e-8), and equals err0 - sum(mu);
  - every case has the gap mu_r / mu_{r+1} >= 10 that makes A B well defined;
  - balancing by powers of two leaves A B bit-identical.
"""
import numpy as np
import pytest

import lrc_ref as L


def fro(a):
    return float(np.linalg.norm(a))


def routes(c):
    E = c["E"].astype(np.float64)
    out = [("gram", L.gram_route(E, c["H"], c["r"]))]
    if c["F"] is not None:
        out.append(("factor", L.factor_route(E, c["F"].astype(np.float64), c["r"])))
    return out


@pytest.mark.parametrize("shape,r", L.CASES, ids=L.CASE_IDS)
def test_routes_agree_with_svd(shape, r):
    c = L.case(shape, r)
    E = c["E"].astype(np.float64)
    A0, B0, info = L.reference(c)
    AB = A0 @ B0
    assert info["rank"] == r
    U, s, _ = np.linalg.svd(E @ L.sqrt_psd(c["H"]), full_matrices=False)
    mu = s * s
    gap = mu[r - 1] / mu[r] if r < mu.size and mu[r] > 0 else np.inf
    assert gap >= 10.0, gap
    for name, (a0, b0, inf) in routes(c):
        err = fro(a0 @ b0 - AB) / fro(E)
        print(f"{shape[0]} r={r} {name}: AB {err:.2e} (bar 1e-10), gap {gap:.1f}")
        assert err <= 1e-10
        assert np.max(np.abs(inf["mu"] - info["mu"])) <= 1e-12 * info["mu"][0]
        assert abs(inf["err0"] - info["err0"]) <= 1e-12 * info["err0"]
        assert inf["rank"] == r
        assert np.max(np.abs(a0.T @ a0 - np.eye(r))) <= 1e-10


def test_cases_take_every_route():
    """m <= p (the m-route) and m > p (the p-route) both occur among the factor
    cases, and one eigenproblem is larger than the eigensolver's one-stage path."""
    took = {s[1] <= s[4] for s, _ in L.CASES if s[3] == "factor"}
    assert took == {True, False}
    assert max(s[1] for s, _ in L.CASES if s[3] == "gram") > 33


@pytest.mark.parametrize("shape,r", L.CASES, ids=L.CASE_IDS)
def test_eckart_young(shape, r):
    c = L.case(shape, r)
    E = c["E"].astype(np.float64)
    A0, B0, info = L.reference(c)
    direct = L.weighted_error(E, A0 @ B0, c["H"])
    assert info["tail"] > 0.0
    assert abs(direct - info["tail"]) <= 1e-10 * info["tail"]
    assert abs(info["err1"] - info["tail"]) <= 1e-10 * info["tail"]
    assert abs(L.weighted_error(E, 0.0 * E, c["H"]) - info["err0"]) <= 1e-10 * info["err0"]
    # no other rank-r correction in the row space of Q does better
    assert direct <= info["err0"]


@pytest.mark.parametrize("shape,r", L.CASES[::4], ids=L.CASE_IDS[::4])
def test_balancing_is_exact(shape, r):
    c = L.case(shape, r)
    A0, B0, _ = L.reference(c)
    A, B = L.balance(A0, B0)
    AB0, AB = A0 @ B0, A @ B
    assert np.array_equal(AB0.view(np.uint64), AB.view(np.uint64))
    for j in range(r):
        ratio = np.abs(B[j]).max() / np.abs(A[:, j]).max()
        assert 0.5 <= ratio <= 2.0, ratio        # within one binade of each other
    assert np.max(np.abs(L.unbalance(A) - A0)) == 0.0


def test_rank_deficient_residual():
    c = L.rank3_case()
    E = c["E"].astype(np.float64)
    A0, B0, info = L.reference(c)
    assert info["rank"] == 3
    assert not A0[:, 3:].any() and not B0[3:].any() and not info["mu"][3:].any()
    a0, b0, inf = L.gram_route(E, c["H"], 8)
    assert inf["rank"] == 3
    assert fro(a0 @ b0 - A0 @ B0) <= 1e-10 * fro(E)
    # all of E's weighted energy is captured (what is left is rounding)
    assert L.weighted_error(E, A0 @ B0, c["H"]) <= 1e-12 * info["err0"]


def test_degenerate_hessian():
    c = L.degenerate_case()
    H = c["H"]
    assert not H[c["dead"]].any() and not H[:, c["dead"]].any()
    for a, b in c["pairs"]:
        assert np.array_equal(H[a], H[b])
    E = c["E"].astype(np.float64)
    A0, B0, info = L.reference(c)
    a0, b0, inf = L.gram_route(E, H, 8)
    assert info["rank"] == inf["rank"] == 8
    assert fro(a0 @ b0 - A0 @ B0) <= 1e-10 * fro(E)
    assert abs(L.weighted_error(E, A0 @ B0, H) - info["tail"]) <= 1e-10 * info["tail"]


def test_sketch_route_matches_gram():
    c = L.sketch_case()
    E = c["E"].astype(np.float64)
    a0, b0, _ = L.factor_route(E, c["F"].astype(np.float64), 8)
    g0, h0, _ = L.gram_route(E, c["H"], 8)
    assert fro(a0 @ b0 - g0 @ h0) <= 1e-10 * fro(E)


# ---------------------------------------------------------------------------
# argument errors of gptq_utils.lowrank_correction (raised before any GPU work)
# ---------------------------------------------------------------------------
def test_lowrank_correction_argument_errors():
    import torch

    import gptq_svd_amd.gptq_utils as g
    E = torch.zeros(8, 16)
    H = torch.eye(16, dtype=torch.float64)
    F = torch.zeros(4, 16, dtype=torch.float64)
    for r in (0, 129, 9):
        with pytest.raises(ValueError, match="r "):
            g.lowrank_correction(E, r, H=H)
    with pytest.raises(ValueError, match="exactly one"):
        g.lowrank_correction(E, 4, H=H, factor=F)
    with pytest.raises(ValueError, match="exactly one"):
        g.lowrank_correction(E, 4)
    with pytest.raises(ValueError, match="perm"):
        g.lowrank_correction(E, 4, H=H, perm=torch.arange(16))
    with pytest.raises(ValueError, match="shape"):
        g.lowrank_correction(E, 4, H=torch.eye(8, dtype=torch.float64))
    with pytest.raises(ValueError, match="matrix"):
        g.lowrank_correction(torch.zeros(8), 1, H=H)
    with pytest.raises(RuntimeError):                      # valid arguments: no CPU fallback
        g.lowrank_correction(E, 4, H=H)


def test_quantize_model_argument_errors(monkeypatch):
    """lowrank is checked before any work: its range, its dtype, and the
    multi-GPU mode."""
    import torch

    from gptq_svd_amd import harness as h
    for bad in (-1, 129):
        with pytest.raises(ValueError, match="lowrank must be in"):
            h.quantize_model(None, [], lowrank=bad)
    with pytest.raises(ValueError, match="lowrank_dtype"):
        h.quantize_model(None, [], lowrank=8, lowrank_dtype=torch.float64)
    monkeypatch.setattr(h, "_world", lambda pg=None: (2, 0))
    with pytest.raises(ValueError, match="lowrank is single-process"):
        h.quantize_model(None, [], lowrank=8)
    with pytest.raises(ValueError, match="single-process"):
        h.quantize_model(None, [], lowrank=8, weight_format="mxfp4")


def test_modules_take_and_refuse_factors():
    """QuantLinear / MXQuantLinear: the optional buffers and their checks."""
    import torch

    from gptq_svd_amd.qlinear import MXQuantLinear, QuantLinear
    q = QuantLinear(64, 32, 4, 32)
    assert q.lr_a is None and q.lr_b is None and "lr_a" not in q.state_dict()
    q = QuantLinear(64, 32, 4, 32, lowrank=4, lowrank_dtype=torch.bfloat16)
    assert q.lr_a.shape == (32, 4) and q.lr_b.shape == (4, 64) and q.lr_a.dtype == torch.bfloat16
    assert {"lr_a", "lr_b"} <= set(q.state_dict()) and "lowrank=4" in repr(q)
    mx = MXQuantLinear(64, 32, lowrank=2)
    assert mx.lr_a.shape == (32, 2) and "lowrank=2" in repr(mx)
    for bad in (129, -1):
        with pytest.raises(ValueError):
            QuantLinear(64, 32, 4, 32, lowrank=bad)
    with pytest.raises(ValueError):
        MXQuantLinear(64, 32, lowrank=4, lowrank_dtype=torch.float64)
    A, B = torch.zeros(32, 4, dtype=torch.float16), torch.zeros(4, 64, dtype=torch.float16)
    m = MXQuantLinear.from_packed(mx.qweight, mx.scales, lowrank=(A, B))
    assert m.lr_a.shape == (32, 4)
    with pytest.raises(ValueError):
        MXQuantLinear.from_packed(mx.qweight, mx.scales, lowrank=(A[:8], B))


def test_checkpoint_carries_the_factors(tmp_path):
    """save_quantized / load_quantized on the CPU: lr_a / lr_b travel, the config
    records the rank, and half a pair is refused."""
    import torch

    from gptq_svd_amd.export import load_quantized, read_quantized, save_quantized
    from gptq_svd_amd.qlinear import QuantLinear
    lin = torch.nn.Sequential(torch.nn.Linear(64, 32, bias=False))
    q = QuantLinear(64, 32, 4, 32)
    A = torch.arange(32 * 4, dtype=torch.float16).reshape(32, 4)
    B = torch.arange(4 * 64, dtype=torch.float16).reshape(4, 64)
    packed = {"0": dict(qweight=q.qweight, qzeros=q.qzeros, scales=q.scales, lr_a=A, lr_b=B)}
    save_quantized(str(tmp_path), lin, packed, 4, 32, False)
    tensors, qc = read_quantized(str(tmp_path))
    assert qc["lowrank"] == 4 and torch.equal(tensors["0.lr_a"], A)
    model = load_quantized(torch.nn.Sequential(torch.nn.Linear(64, 32, bias=False)), str(tmp_path))
    assert isinstance(model[0], QuantLinear)
    assert torch.equal(model[0].lr_a, A) and torch.equal(model[0].lr_b, B)
    with pytest.raises(ValueError, match="come together"):
        save_quantized(str(tmp_path / "bad"), lin, {"0": dict(packed["0"], lr_b=None)}, 4, 32,
                       False)


def test_abi_rejects_bad_arguments():
    """tg_lrc_factor checks its arguments before any device work."""
    import ctypes

    from gptq_svd_amd import _lib as lib
    one = ctypes.c_void_p(256)

    def rc(m=8, n=16, se=16, f_dtype=lib.TG_F64, p=4, sf=16, perm=None, gram=0, r=4, sa=4, sb=16,
           ab=lib.TG_F32, E=one, F=one):
        return lib.lib.tg_lrc_factor(None, E, m, n, se, F, f_dtype, p, sf, perm, gram, r, one, sa,
                                     one, sb, ab, one, one, one, one, 0)

    assert rc(E=None) == -2
    assert rc(se=15) == -5
    assert rc(F=None) == -6
    assert rc(f_dtype=lib.TG_F16) == -7
    assert rc(gram=1, f_dtype=lib.TG_F32) == -7
    assert rc(p=0) == -8
    assert rc(sf=15) == -9
    assert rc(gram=1, perm=one) == -10
    assert rc(gram=2) == -11
    for r in (0, 129, 9):
        assert rc(r=r) == -12
    assert rc(sa=3) == -14
    assert rc(sb=15) == -16
    assert rc(ab=lib.TG_F16) == -17
    assert rc() == -99 and "workspace" in lib.last_error()
    assert lib.lib.tg_lrc_workspace_size(12288, 4096, 4096, 32, 0) > 12288 * 4096 * 8
    assert lib.lib.tg_lrc_workspace_size(0, 16, 4, 4, 0) == 0
