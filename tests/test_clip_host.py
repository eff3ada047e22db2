"""CPU side of the clip search (A7c): the numpy restatement of the contract
(tests/clip_ref.py) against the oracle's find_params, the ambiguity census
that keeps test_gpu_clip.py's cap honest, the argument checks of
tg_group_params_clip, the Quantizer's constructor, and the end-to-end
experiment of DESIGN.md at one pinned setting."""
import ctypes
import os

import numpy as np
import pytest

import clip_ref
from conftest import ROOT

LIB = os.path.join(ROOT, "gptq-svd_amd", "libtruncgptq.so")
CASES = [(s, b, sym) for s in clip_ref.SHAPES for b in clip_ref.BITS for sym in (False, True)]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32),
                                                                        b.view(np.uint32))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "gptq-svd_amd"), "-j8"], check=True)
    lib = ctypes.CDLL(LIB)
    lib.tg_last_error.restype = ctypes.c_char_p
    return lib


@pytest.mark.parametrize("shape", clip_ref.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_step0_is_find_params(oracle_mod, shape):
    """steps = 0 is today's find_params bit for bit, and the chosen objective
    never exceeds candidate 0's."""
    m, n, group = shape
    W = clip_ref.clip_input(m, n, group)
    for bits in clip_ref.BITS:
        for sym in (False, True):
            s_ref, z_ref = oracle_mod.find_params(W, bits, group, sym)
            r0 = clip_ref.clip_search(W, None, bits, group, sym, grid=100, steps=0)
            assert r0["J"].shape[2] == 1 and not r0["choice"].any()
            assert bits_equal(r0["s"][:, :, 0], s_ref), (shape, bits, sym)
            assert bits_equal(r0["z"][:, :, 0], z_ref), (shape, bits, sym)
            for weighted in (False, True):
                _, _, ref = clip_ref.case(m, n, group, bits, sym, weighted)
                assert bits_equal(ref["s"][:, :, 0], s_ref) and bits_equal(ref["z"][:, :, 0], z_ref)
                chosen = np.take_along_axis(ref["J"], ref["choice"][:, :, None].astype(np.int64),
                                            axis=2)[:, :, 0]
                assert np.all(chosen <= ref["J"][:, :, 0])
                assert np.all(np.isfinite(ref["J"]))


def test_ambiguity_census_is_zero():
    """No group of the GPU test's inputs has two distinct candidates within
    1e-9 relative at the minimum, so its 1 % cap excuses nothing."""
    groups = amb = 0
    for (m, n, group), bits, sym in CASES:
        for weighted in (False, True):
            _, _, ref = clip_ref.case(m, n, group, bits, sym, weighted)
            a = clip_ref.ambiguous(ref)
            groups += a.size
            amb += int(a.sum())
    print(f"ambiguous groups: {amb} of {groups}")
    assert groups == 6928
    assert amb == 0


P = ctypes.c_void_p(16)
GOOD = dict(W=P, m=4, n=256, stride_w=256, col_weight=None, group=128, w_bits=4, sym=0, grid=100,
            steps=80, scale=P, zero=P, choice=None, objective=None)
BAD = [("W", None, 2, b"W"), ("m", 0, 3, b"m"), ("n", 0, 4, b"n"), ("stride_w", 255, 5, b"stride_w"),
       ("group", 100, 7, b"group"), ("w_bits", 1, 8, b"w_bits"), ("w_bits", 9, 8, b"w_bits"),
       ("grid", 0, 10, b"grid"), ("steps", -1, 11, b"steps"), ("steps", 100, 11, b"steps"),
       ("scale", None, 12, b"scale"), ("zero", None, 13, b"zero")]


@pytest.mark.parametrize("arg,value,index,word", BAD, ids=[f"{a}={v}" for a, v, _, _ in BAD])
def test_argument_errors_without_gpu(lib, arg, value, index, word):
    """Each bad argument is rejected with its index before any device work
    (null stream, pointers that are never dereferenced)."""
    fn = lib.tg_group_params_clip
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                   ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                   ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p]
    a = dict(GOOD)
    a[arg] = value
    rc = fn(None, *a.values())
    msg = lib.tg_last_error()
    assert rc == -index, (rc, msg)
    assert f"argument {index}".encode() in msg and word in msg, msg


def test_quantizer_arguments():
    import torch
    import gptq_svd_amd.gptq_utils as g
    with pytest.raises(ValueError):
        g.Quantizer(clip_steps=100, clip_grid=100)
    with pytest.raises(ValueError):
        g.Quantizer(clip_steps=-1)
    q = g.Quantizer(4, 128, False)                      # the first three stay positional
    assert (q.w_bits, q.group_size, q.sym, q.clip_search) == (4, 128, False, False)
    q = g.Quantizer(4, 128, False, clip_search=True, col_weight=torch.ones(128))
    assert (q.clip_grid, q.clip_steps) == (100, 80)
    with pytest.raises(RuntimeError):
        q.find_params(torch.zeros(4, 128))              # no CPU fallback with the search either


def test_weighted_search_helps_end_to_end(oracle_mod, monkeypatch):
    """The oracle's solve (process_hessian_alt, energy rule 1e-4; gptq_fwrd,
    block 128) at 3-bit sym g128 on the pinned problem of clip_ref: with
    scales from the search weighted by diag(H) the proxy error
    ||(W - Wq) X^T||_F is below 0.85 x the min/max solve's."""
    bits, group, sym = 3, 128, True
    X, W = clip_ref.quality_problem(seed=11)
    acc = oracle_mod.HessianAccumulator(X.shape[1])
    acc.add_batch(X)
    H = acc.get_hessian()
    f = oracle_mod.process_hessian_alt(H, 1e-4, "energy")

    def solve():
        Wq, _ = oracle_mod.gptq_fwrd(W, f.U, f.perm, bits, group, sym, 128, impl="c")
        return clip_ref.proxy_error(W, Wq, X)

    plain = solve()
    ref = clip_ref.clip_search(W, np.diag(H).astype(np.float32), bits, group, sym)
    pick = lambda a: np.take_along_axis(a, ref["choice"][:, :, None].astype(np.int64),
                                        axis=2)[:, :, 0].copy()

    def searched(W_, bits_, group_, sym_):
        assert (bits_, group_, sym_) == (bits, group, sym) and np.array_equal(W_, W)
        return pick(ref["s"]), pick(ref["z"])

    monkeypatch.setattr(oracle_mod, "find_params", searched)
    clipped = solve()
    print(f"proxy error: min/max {plain:.5f}, weighted search {clipped:.5f}, "
          f"ratio {clipped / plain:.3f}")
    assert clipped < 0.85 * plain
