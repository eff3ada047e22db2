"""CPU: the host reference of the MXFP4 format (mx_ref.py) proved against
definitions that do not share its code, and the argument checks of the new C
entry points (no device work: there is no GPU here)."""
import ctypes
import json

import numpy as np
import pytest
import torch

import mx_ref as R
from conftest import load_golden

F32 = np.float32


# ---- element rule -------------------------------------------------------------
def nearest_even(t):
    """(index, negative) of the E2M1 value nearest to t by exact arithmetic:
    distances in float64 (exact for float32 t), ties to the even index,
    saturating at 6."""
    grid = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    a = abs(float(t))
    best = min(range(8), key=lambda i: (abs(a - grid[i]), i % 2))
    return best, (float(t) < 0 and best != 0)


@pytest.mark.parametrize("E", [-126, -3, 0, 5, 120])
def test_ties_neighbours_and_saturation(E):
    s = R.pow2(E)
    t = R.tie_points()
    w = (t * s).astype(F32)                      # exact unless it falls among the subnormals
    exact = E >= -124
    assert np.array_equal((w / s).astype(F32), t) == exact
    t = (w / s).astype(F32)
    qv, code = R.quantize_elements(w, np.full_like(w, s))
    for ti, q, c in zip(t, qv, code):
        idx, neg = nearest_even(ti)
        assert int(c) == (idx | (8 if neg else 0)), (ti, c)
        want = F32(R.GRID[idx]) * s
        assert q == (-want if neg else want) and (idx != 0 or not np.signbit(q)), (ti, q)
    assert 8 not in set(code.tolist())
    # the exact ties go to the even code, their neighbours to either side
    for tie, (lo, hi) in zip(R.TIES, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7)]):
        if not exact:
            break
        tie = F32(tie)
        trio = np.array([np.nextafter(tie, F32(0)), tie, np.nextafter(tie, F32(100))], dtype=F32)
        for sign in (1, -1):
            _, c = R.quantize_elements(sign * trio * s, np.full(3, s, dtype=F32))
            even = lo if lo % 2 == 0 else hi
            assert [int(x) & 7 for x in c] == [lo, even, hi]
            assert all((int(x) >> 3) == (1 if sign < 0 and (int(x) & 7) else 0) for x in c)
    # saturation
    _, c = R.quantize_elements(np.array([6.0, 7.0, 100.0, -100.0], dtype=F32) * s,
                               np.full(4, s, dtype=F32))
    assert c.tolist() == [7, 7, 7, 15]


def test_scale_rule_points():
    a = np.array([4.0, np.nextafter(F32(4), F32(0)), 6.0, 0.0, 1e-40, 3e38, 1.0, 0.75,
                  np.finfo(F32).tiny, np.finfo(F32).max], dtype=F32)
    E = R.scale_exponent(a)
    assert E.tolist() == [0, -1, 0, -126, -126, 125, -2, -3, -126, 125]
    W = np.zeros((len(a), 32), dtype=F32)
    W[np.arange(len(a)), np.arange(len(a))] = a * np.where(np.arange(len(a)) % 2, -1, 1)
    scale, byte = R.group_scales(W)
    assert byte[:, 0].tolist() == [e + 127 for e in E.tolist()]
    assert np.array_equal(scale[:, 0], np.ldexp(1.0, E).astype(F32))
    assert byte.min() >= 1 and byte.max() <= 252          # 255 (NaN) is never written
    assert np.all(scale >= np.finfo(F32).tiny)            # always a normal fp32
    # against log2 in float64 on random magnitudes (exact powers of two included)
    rng = np.random.default_rng(0)
    r = np.concatenate([np.exp(rng.uniform(-80, 80, 4000)), 2.0 ** rng.integers(-120, 120, 200)])
    r = r.astype(F32)
    want = np.maximum(np.floor(np.log2(r.astype(np.float64))).astype(np.int64) - 2, -126)
    assert np.array_equal(R.scale_exponent(r), want)


def test_reciprocal_multiply_equals_division():
    rng = np.random.default_rng(1)
    t = np.concatenate([R.tie_points(), rng.uniform(-8, 8, 400).astype(F32),
                        (rng.standard_normal(200) * 1e-3).astype(F32)])
    t = t[np.abs(t) <= 7]                                  # 7 * 2^125 is finite
    for E in range(-126, 126):
        s = R.pow2(E)
        assert s * (F32(1.0) / s) == F32(1.0) and np.isfinite(F32(1.0) / s)
        w = (t * s).astype(F32)
        sv = np.full_like(w, s)
        qa, ca = R.quantize_elements(w, sv, recip=False)
        qb, cb = R.quantize_elements(w, sv, recip=True)
        assert np.array_equal(qa.view(np.int32), qb.view(np.int32)) and np.array_equal(ca, cb), E


def test_encode_decode_idempotent():
    rng = np.random.default_rng(2)
    W = (rng.standard_normal((24, 96)) * np.exp(rng.uniform(-30, 30, (24, 1)))).astype(F32)
    W[3, :32] = 0.0                                        # an all-zero group
    Wq, codes, scale, byte = R.rtn(W)
    assert np.array_equal(R.decode32(codes, R.expand(byte)).view(np.int32), Wq.view(np.int32))
    assert 8 not in set(codes.reshape(-1).tolist())
    Wq2, codes2, scale2, byte2 = R.rtn(Wq)
    assert np.array_equal(Wq2.view(np.int32), Wq.view(np.int32))
    assert np.array_equal(codes2, codes)
    nz = np.abs(Wq).reshape(24, 3, 32).max(axis=2) > 0     # a group rounded to zero re-scales
    assert np.array_equal(byte2[nz], byte[nz])
    # every byte decodes; fp16 overflows for large scales, bf16 does not
    allb = np.arange(255, dtype=np.uint8)
    six = R.decode(np.full(255, 7), allb, "f32")
    # 6 * 2^125 (byte 252, the largest the solver writes) is finite, 6 * 2^126 is not
    assert torch.isfinite(six[:253]).all() and torch.isinf(six[253:]).all()
    assert torch.isfinite(R.decode(np.full(255, 5), allb, "f32")[:254]).all()  # 3 * 2^126
    assert float(R.decode(np.array([1]), np.array([0]), "f32")[0]) == 2.0 ** -128
    h = R.decode(np.full(255, 7), allb, "f16")
    assert torch.isfinite(h[:141]).all() and torch.isinf(h[141:]).all()
    assert torch.isfinite(R.decode(np.full(255, 7), allb, "bf16")[:253]).all()


# ---- the loops ------------------------------------------------------------------
def test_loops_reduce_to_rtn_without_propagation():
    """With U = I nothing propagates: both loops and the tail are plain RTN."""
    rng = np.random.default_rng(3)
    W = rng.standard_normal((6, 64)).astype(F32)
    perm = rng.permutation(64)
    want = R.rtn(W)
    for loop in (False, True):
        for k in (64, 40):
            Wq, codes, scale, byte = R.gptq_fwrd_mx(W, np.eye(64, dtype=F32)[:k], perm, 24, loop)
            assert np.array_equal(Wq.view(np.int32), want[0].view(np.int32))
            assert np.array_equal(codes, want[1]) and np.array_equal(byte, want[3])


def test_shape_one_plants_what_it_says():
    W, U, perm, c0, planted = R.shape_one()
    assert W.shape == (17, 160) and U.shape == (112, 160) and c0 == perm[0]
    scale, byte = R.group_scales(W)
    assert np.all(byte[:, c0 // 32] == 127)                     # a in [4, 8): scale 1
    assert set(np.abs(planted[:14]).tolist()) == set(R.TIES)
    for loop in (False, True):
        Wq, codes, _, _ = R.gptq_fwrd_mx(W, U, perm, 48, loop)
        want_q, want_c = R.quantize_elements(planted, np.ones(17, dtype=F32))
        assert np.array_equal(Wq[:, c0].view(np.int32), want_q.view(np.int32))
        assert np.array_equal(codes[:, c0], want_c)
        assert not np.array_equal(codes, R.rtn(W)[1])          # the propagation moved codes
        assert np.array_equal(R.decode32(codes, R.expand(byte)).view(np.int32), Wq.view(np.int32))


def test_exact_gemm_cases_are_exact():
    for T in (1, 4, 5, 16, 33):
        c = R.exact_gemm_case(96, 160, T, seed=T)
        assert c["abs_int"].max() + 100 < 2 ** 24 and set(c["byte"].reshape(-1).tolist()) == {127}
    c = R.exact_gemm_case(4416, 2048, 4, seed=9, distinct=True)
    assert c["abs_int"].max() < 2 ** 24
    assert np.all(c["byte"][:, 1:] != c["byte"][:, :-1])       # consecutive units differ
    for dt in ("f16", "bf16"):                                  # the operands are exact in 16 bits
        w = torch.from_numpy(c["w_int"][:64].astype(F32))
        assert torch.equal(w.to(R.TDT[dt]).float(), w)


def tiny_first_group():
    """Layer 0's attention inputs of the tiny random Qwen3 golden, from the
    unquantised model on the CPU: (golden, H float64, {name: W})."""
    from transformers import Qwen3Config, Qwen3ForCausalLM
    d = load_golden("h_qwen3tiny_eigh_w4a")
    cfg = Qwen3Config(**json.loads(str(d["config"])))
    cfg._attn_implementation = "eager"
    m = Qwen3ForCausalLM(cfg).float().eval()
    m.load_state_dict({k[len("init/"):]: torch.from_numpy(d[k]) for k in d
                       if k.startswith("init/")})
    layer = m.model.layers[0]
    with torch.no_grad():
        x = layer.input_layernorm(m.model.embed_tokens(torch.from_numpy(d["ids"])))
    x = x.reshape(-1, x.shape[-1]).double().numpy()
    W = {n: getattr(layer.self_attn, n).weight.detach().numpy() for n in ("q_proj", "k_proj")}
    return d, x.T @ x / x.shape[0], W


def test_propagation_beats_plain_casting(oracle_mod):
    """The point of the solver: pushing the error through the E2M1 grid gives a
    smaller prediction error than plain MX casting (test_gpu_mx.py asserts the
    same of the GPU run on this layer)."""
    d, H, Ws = tiny_first_group()
    f = oracle_mod.process_hessian_alt(H, float(d["eps"]), str(d["method"]))
    for name, W in Ws.items():
        Wq = R.gptq_fwrd_mx(W, f.U, f.perm, 1024)[0]
        e_solver = oracle_mod.relative_prediction_error(W, Wq, f.R_x, f.perm)
        e_rtn = oracle_mod.relative_prediction_error(W, R.rtn(W)[0], f.R_x, f.perm)
        print(f"{name}: solver {e_solver:.4f}, plain casting {e_rtn:.4f}")
        assert e_solver < e_rtn


# ---- argument errors of the new entry points ------------------------------------
@pytest.fixture(scope="module")
def L():
    import gptq_svd_amd._lib as lib
    return lib


P = ctypes.c_void_p(64)


def test_group_params_mx_arguments(L):
    f = L.lib.tg_group_params_mx
    assert f(None, None, 4, 64, 64, 1, P, P) == -2 and "null" in L.last_error()
    assert f(None, P, 0, 64, 64, 1, P, P) == -3
    assert f(None, P, 4, 48, 48, 1, P, P) == -4 and "multiple of 32" in L.last_error()
    assert f(None, P, 4, 64, 63, 1, P, P) == -5
    assert f(None, P, 4, 64, 64, 0, P, P) == -6 and "fmt" in L.last_error()
    assert f(None, P, 4, 64, 64, 1, None, P) == -7
    assert f(None, P, 4, 64, 64, 1, P, None) == -8


def test_quantize_mx_arguments(L):
    def f(W=P, m=4, n=64, U=P, k=64, ldu=64, perm=P, scale=P, fmt=1, loop=0, block=32, Wq=P):
        return L.lib.tg_gptq_quantize_mx(None, W, m, n, U, k, ldu, perm, scale, fmt, loop, block,
                                         Wq, None, None, 0)
    assert f(W=None) == -2
    assert f(n=80) == -4 and "multiple of 32" in L.last_error()
    assert f(U=None) == -5
    assert f(k=65) == -6 and f(k=0) == -6
    assert f(ldu=63) == -7
    assert f(perm=None) == -8
    assert f(scale=None) == -9
    assert f(fmt=7) == -10 and "fmt" in L.last_error()
    assert f(loop=2) == -11
    assert f(block=0) == -12 and f(block=4096) == -12
    assert f(Wq=None) == -13


def test_pack_and_dequant_mx_arguments(L):
    f = L.lib.tg_pack_e8m0
    assert f(None, None, 8, 2, P) == -2 and f(None, P, 0, 2, P) == -3
    assert f(None, P, 8, 0, P) == -4 and f(None, P, 8, 2, None) == -5

    def dq(qw=P, sc=P, fmt=1, m=8, n=64, out=P, dt=L.TG_F16, ldo=64):
        return L.lib.tg_dequant_mx(None, qw, sc, fmt, m, n, out, dt, ldo)
    assert dq(qw=None) == -2 and dq(sc=None) == -3
    assert dq(fmt=0) == -4 and "fmt" in L.last_error()
    assert dq(m=12) == -5 and "multiple of 32" in L.last_error()     # m * 4 % 32 != 0
    assert dq(n=48) == -6 and "multiple of 32" in L.last_error()
    assert dq(out=None) == -7
    assert dq(dt=L.TG_F64) == -8 and "out_dtype" in L.last_error()
    assert dq(ldo=63) == -9


def test_qgemm_mx_arguments(L, monkeypatch):
    def g(X=P, xdt=L.TG_F16, T=3, ldx=64, qw=P, sc=P, fmt=1, m=8, n=64, bias=None, bdt=0, Y=P,
          ydt=L.TG_F16, ldy=8, ws=None):
        return L.lib.tg_qgemm_mx(None, X, xdt, T, ldx, qw, sc, fmt, m, n, bias, bdt, Y, ydt, ldy,
                                 ws, 0)
    assert g(X=None) == -2
    assert g(xdt=L.TG_F32) == -3 and "x_dtype" in L.last_error()
    assert g(T=0) == -4
    assert g(ldx=63) == -5
    assert g(qw=None) == -6 and g(sc=None) == -7
    assert g(fmt=2) == -8 and "fmt" in L.last_error()
    assert g(m=12) == -9 and "multiple of 32" in L.last_error()
    assert g(n=80) == -10 and "multiple of 32" in L.last_error()
    assert g(bias=P, bdt=L.TG_F64) == -12
    assert g(Y=None) == -13
    assert g(xdt=L.TG_F16, ydt=L.TG_BF16) == -14
    assert g(ldy=7) == -15
    assert g() == -16 and "workspace" in L.last_error()               # the gemv regime needs one
    monkeypatch.setenv("TG_QGEMM", "gemv")
    assert g(T=17) == -4 and "gemv" in L.last_error()


def test_python_argument_errors():
    from gptq_svd_amd.gptq_utils import Quantizer
    from gptq_svd_amd.harness import quantize_model
    from gptq_svd_amd.qlinear import MXQuantLinear, dequantize_packed_mx
    Quantizer(4, 32, weight_format="mxfp4")
    for kw in (dict(w_bits=3, group_size=32), dict(w_bits=4, group_size=128),
               dict(w_bits=4, group_size=32, clip_search=True)):
        with pytest.raises(ValueError):
            Quantizer(weight_format="mxfp4", **kw)
    with pytest.raises(ValueError):
        Quantizer(4, 32, weight_format="nvfp4")
    # the unsupported combinations raise before any work (no model is touched)
    with pytest.raises(ValueError, match="clip_search"):
        quantize_model(None, [], weight_format="mxfp4", clip_search=True)
    with pytest.raises(ValueError, match="weight_format"):
        quantize_model(None, [], weight_format="mxfp6")
    with pytest.raises(ValueError):
        MXQuantLinear(48, 8)
    with pytest.raises(ValueError, match="uint8"):
        dequantize_packed_mx(torch.zeros(8, 8, dtype=torch.int32), torch.zeros(2, 8))
    with pytest.raises(RuntimeError):                                  # no CPU fallback
        dequantize_packed_mx(torch.zeros(8, 8, dtype=torch.int32),
                             torch.zeros(2, 8, dtype=torch.uint8))
