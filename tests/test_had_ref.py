"""CPU: the numpy restatement of the Hadamard rotation (had_ref.py) against the
explicit kron / Sylvester product, the quality condition of the rotation on the
oracle, and the host-side checks of the Python layers (no GPU)."""
import json
import os

import numpy as np
import pytest
import torch

import had_ref as hr

U32, U64 = 2.0 ** -24, 2.0 ** -53


@pytest.mark.parametrize("b", hr.BLOCKS)
def test_integer_data_equals_the_kron_product(b):
    """|x| <= 8 integers: every partial sum is an integer below 2^24, so f32 and
    f64 are exact up to the one multiply by c (exact when c is a power of two,
    one rounding otherwise)."""
    n = b if b >= 1024 else 3 * b
    x = hr.integer_rows(3, n, b)
    words = hr.pack_signs(hr.mixed_signs(n, b, 1))
    Q = hr.q_matrix(n, b, words)
    unscaled = x @ (Q * np.sqrt(b))            # integers, exact in float64
    for ct in (np.float32, np.float64):
        y = hr.rows_np(x.astype(ct), b, words)
        assert y.dtype == ct
        assert np.array_equal(y, unscaled.astype(ct) * hr.scale_of(b, ct))
        back = hr.rows_np(x.astype(ct), b, words, inverse=True)
        assert np.array_equal(back, (x @ (Q.T * np.sqrt(b))).astype(ct) * hr.scale_of(b, ct))


@pytest.mark.parametrize("b", hr.BLOCKS)
def test_random_data_within_the_butterfly_bound(b):
    """|R(x) - x Q| <= log2(b) u |x|_1 / sqrt(b), |x|_1 of the element's block:
    log2 b rounded additions on partial sums that the block's 1-norm bounds."""
    n = 2 * b
    rng = np.random.default_rng(b)
    x = rng.standard_normal((4, n))
    words = hr.pack_signs(hr.random_signs(n, 3))
    Q = hr.q_matrix(n, b, words)
    for ct, u in ((np.float32, U32), (np.float64, U64)):
        xc = x.astype(ct)
        want = xc.astype(np.float64) @ Q
        l1 = np.abs(xc.astype(np.float64)).reshape(4, n // b, b).sum(axis=2)
        bound = np.log2(b) * u * np.repeat(l1, b, axis=1) / np.sqrt(b)
        for inverse in (False, True):
            ref = want if not inverse else xc.astype(np.float64) @ Q.T
            err = np.abs(hr.rows_np(xc, b, words, inverse).astype(np.float64) - ref)
            assert np.all(err <= bound), float((err / bound).max())


@pytest.mark.parametrize("b", [64, 256, 1024, 4096])
def test_round_trip_is_exact_when_c_is_a_power_of_two(b):
    x = hr.integer_rows(2, 2 * b if b < 4096 else b, 5).astype(np.float32)
    words = hr.pack_signs(hr.random_signs(x.shape[1], 9))
    y = hr.rows_np(x, b, words)
    assert np.array_equal(hr.rows_np(y, b, words, inverse=True), x)
    t = hr.rows(torch.from_numpy(x).half(), b, words, out="f32")
    assert torch.equal(hr.rows(t, b, words, inverse=True, out="f16").float(), torch.from_numpy(x))


def test_sign_bits_round_trip():
    s = hr.random_signs(96, 0)
    w = hr.pack_signs(s)
    assert w.dtype == np.int32 and w.shape == (3,)
    assert np.array_equal(hr.unpack_signs(w, 96), s)
    e = np.ones(64)
    e[31] = e[32 + 5] = -1
    assert hr.pack_signs(e).tolist() == [-2 ** 31, 1 << 5]
    assert np.array_equal(hr.unpack_signs(None, 32), np.ones(32))
    m = hr.mixed_signs(256, 128)
    assert m[2] != m[130] and m[0] == 1 and m[1] == -1


def test_output_rounding_is_one_rne():
    x = torch.randn(3, 64, generator=torch.Generator().manual_seed(0))
    y32 = hr.rows(x, 32, out="f32")
    for dt in ("f16", "bf16"):
        assert torch.equal(hr.rows(x, 32, out=dt), y32.to(hr.TDT[dt]))


@pytest.mark.parametrize("n,b", [(32, 32), (96, 32), (256, 128), (512, 256)])
def test_two_sided_form(n, b):
    from mx_ref import hessian_case
    H = hessian_case(n, 2 * n, 1)
    words = hr.pack_signs(hr.random_signs(n, 2))
    S = hr.sym(H, b, words)
    assert np.array_equal(S, S.T)
    Q = hr.q_matrix(n, b, words)
    want = Q.T @ H @ Q
    assert np.linalg.norm(S - want) <= 1e-13 * np.linalg.norm(want)
    # the objective is invariant: tr(E H E^T) = tr(E' H' E'^T)
    E = np.random.default_rng(0).standard_normal((5, n))
    a, c = hr.weighted_error(E, 0 * E, H), hr.weighted_error(E @ Q, 0 * E, S)
    assert abs(a - c) <= 1e-12 * a


def _solve(o, W, H, bits, group):
    f = o.process_hessian_alt(H, 1e-4, "energy")
    Wq, _ = o.gptq_fwrd(W, f.U, f.perm, bits, group, False, 1024, gemm="fma", impl="c")
    return Wq, f.k


def test_quality_condition(oracle_mod):
    """The case test_gpu_had_solver.py asserts a factor 2 on: the oracle alone
    gives at least 4 (int4 g128, 32 x 256, four columns x 30, b = 128)."""
    q = hr.QUALITY
    W, H, words = hr.quality_case()
    Wq, k = _solve(oracle_mod, W, H, q["bits"], q["group"])
    Wr = hr.rows_np(W, q["b"], words)
    Hr = hr.sym(H, q["b"], words)
    Wqr, kr = _solve(oracle_mod, Wr, Hr, q["bits"], q["group"])
    plain, rot = hr.weighted_error(W, Wq, H), hr.weighted_error(Wr, Wqr, Hr)
    print(f"weighted error {plain:.4e} unrotated, {rot:.4e} rotated, ratio {plain / rot:.2f}, "
          f"k {k} / {kr}")
    assert plain / rot >= 4.0


# ---------------------------------------------------------------------------
# host-only checks of the Python layers
# ---------------------------------------------------------------------------
def test_auto_block():
    import gptq_svd_amd.gptq_utils as g
    ab = g.HadamardRotation.auto_block
    assert [ab(n) for n in (32, 96, 128, 160, 4096, 11008, 12288, 28672, 8192)] == \
        [32, 32, 128, 32, 4096, 256, 4096, 4096, 4096]
    for n in (0, 16, 48, 100, 4104):
        with pytest.raises(ValueError):
            ab(n)


def test_rotation_argument_validation_and_cpu_refusal():
    import gptq_svd_amd.gptq_utils as g
    for n, b in ((128, 48), (128, 16), (96, 64), (8192, 8192), (100, 32)):
        with pytest.raises(ValueError):
            g.HadamardRotation(n, b, seed=0, device="cpu")
    with pytest.raises(ValueError):
        g.HadamardRotation(64, 32, device="cpu")                       # neither seed nor signs
    with pytest.raises(ValueError):
        g.HadamardRotation(64, 32, seed=0, sign_bits=torch.zeros(2, dtype=torch.int32),
                           device="cpu")
    with pytest.raises(ValueError):
        g.HadamardRotation(64, 32, sign_bits=torch.zeros(3, dtype=torch.int32), device="cpu")
    with pytest.raises(ValueError):
        g.HadamardRotation(64, 32, sign_bits=torch.zeros(2, dtype=torch.int64), device="cpu")
    r = g.HadamardRotation(64, 32, seed=0, device="cpu")
    with pytest.raises(RuntimeError):
        r.rows(torch.zeros(2, 64))
    with pytest.raises(RuntimeError):
        r.hessian_(torch.zeros(64, 64, dtype=torch.float64))


def test_seed_fixes_the_signs():
    import gptq_svd_amd.gptq_utils as g
    a = g.HadamardRotation(256, 128, seed=5, device="cpu").sign_bits
    b = g.HadamardRotation(256, 128, seed=5, device="cpu").sign_bits
    c = g.HadamardRotation(256, 128, seed=6, device="cpu").sign_bits
    assert a.dtype == torch.int32 and tuple(a.shape) == (8,)
    assert torch.equal(a, b) and not torch.equal(a, c)
    # the documented draw: bit j of word i = (randint(0, 2, (n,)) of the seeded CPU generator)[32 i + j]
    bits = torch.randint(0, 2, (256,), generator=torch.Generator().manual_seed(5)).numpy()
    assert np.array_equal(a.numpy(), hr.pack_signs(np.where(bits == 1, -1.0, 1.0)))
    s = np.where(bits == 1, -1.0, 1.0)
    assert 64 < (s < 0).sum() < 192


def test_qlinear_hadamard_refuses_cpu_and_bad_blocks():
    from gptq_svd_amd import qlinear
    with pytest.raises(RuntimeError):
        qlinear.hadamard(torch.zeros(2, 64), 32, None)
    with pytest.raises(ValueError):
        qlinear.QuantLinear(96, 32, 4, 32, rotate_block=64)
    with pytest.raises(ValueError):
        qlinear.MXQuantLinear(96, 32, rotate_block=48)
    q = qlinear.QuantLinear(96, 32, 4, 32, rotate_block=32)
    assert q.had_sign.dtype == torch.int32 and tuple(q.had_sign.shape) == (3,)
    assert "had_sign" in q.state_dict() and q.rotate_block == 32
    p = qlinear.MXQuantLinear(96, 32)
    assert p.had_sign is None and p.rotate_block == 0 and "had_sign" not in p.state_dict()


class _Two(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(64, 32, bias=False)
        self.b = torch.nn.Linear(96, 32, bias=True)


@pytest.mark.parametrize("fmt", ["int", "mxfp4"])
def test_export_config_round_trip(tmp_path, fmt):
    """save_quantized writes <name>.had_sign and the "rotation" block, and
    load_quantized builds rotated modules from them; a checkpoint without the
    key loads into unrotated modules, as before."""
    from gptq_svd_amd import export, qlinear
    gen = torch.Generator().manual_seed(0)

    def packed_of(n, m):
        if fmt == "mxfp4":
            return dict(qweight=torch.randint(-2 ** 31, 2 ** 31 - 1, (n // 8, m), generator=gen,
                                              dtype=torch.int64).to(torch.int32),
                        qzeros=None,
                        scales=torch.randint(120, 130, (n // 32, m), generator=gen,
                                             dtype=torch.int64).to(torch.uint8))
        return dict(qweight=torch.randint(-2 ** 31, 2 ** 31 - 1, (n * 4 // 32, m), generator=gen,
                                          dtype=torch.int64).to(torch.int32),
                    qzeros=torch.randint(0, 2 ** 31 - 1, (n // 32, m * 4 // 32), generator=gen,
                                         dtype=torch.int64).to(torch.int32),
                    scales=torch.rand(n // 32, m, generator=gen).half())

    sa = torch.tensor(hr.pack_signs(hr.random_signs(64, 0)))
    sb = torch.tensor(hr.pack_signs(hr.random_signs(96, 1)))
    packed = {"a": dict(packed_of(64, 32), had_sign=sa, had_block=64),
              "b": dict(packed_of(96, 32), had_sign=sb, had_block=32)}
    path = str(tmp_path / "rot")
    export.save_quantized(path, _Two(), packed, 4, 32, True, weight_format=fmt)
    tensors, qc = export.read_quantized(path)
    assert qc["rotation"] == {"kind": "hadamard", "blocks": {"a": 64, "b": 32}}
    assert torch.equal(tensors["a.had_sign"], sa) and tensors["b.had_sign"].dtype == torch.int32
    model = export.load_quantized(_Two(), path)
    cls = qlinear.MXQuantLinear if fmt == "mxfp4" else qlinear.QuantLinear
    assert isinstance(model.a, cls) and model.a.rotate_block == 64 and model.b.rotate_block == 32
    assert torch.equal(model.b.had_sign, sb) and torch.equal(model.a.qweight, packed["a"]["qweight"])

    # one rotated, one not
    path1 = str(tmp_path / "half")
    export.save_quantized(path1, _Two(), {"a": packed["a"], "b": packed_of(96, 32)}, 4, 32, True,
                          weight_format=fmt)
    model = export.load_quantized(_Two(), path1)
    assert model.a.rotate_block == 64 and model.b.rotate_block == 0 and model.b.had_sign is None

    # without rotation: no key, no tensors
    path0 = str(tmp_path / "plain")
    export.save_quantized(path0, _Two(), {k: packed_of(n, 32) for k, n in (("a", 64), ("b", 96))},
                          4, 32, True, weight_format=fmt)
    tensors, qc = export.read_quantized(path0)
    assert "rotation" not in qc and not [k for k in tensors if k.endswith("had_sign")]
    model = export.load_quantized(_Two(), path0)
    assert model.a.rotate_block == 0 and model.a.had_sign is None

    # a sign tensor the config does not announce, and the reverse, are errors
    with open(os.path.join(path, "quantize_config.json")) as f:
        qc = json.load(f)
    del qc["rotation"]["blocks"]["b"]
    with open(os.path.join(path, "quantize_config.json"), "w") as f:
        json.dump(qc, f)
    with pytest.raises((KeyError, ValueError)):
        export.load_quantized(_Two(), path)
