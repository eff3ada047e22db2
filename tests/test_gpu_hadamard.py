"""GPU: tg_hadamard and tg_hadamard_sym against the numpy restatement
(had_ref.py, proved in test_had_ref.py): bit-equal on random data, exact on
integer data, over every block width (in-wave widths, the wave boundary at 512,
the LDS regime above), several blocks per row, odd row counts, every type pair,
signs, the inverse, in place, padded strides inside sentinel images, the scalar
path of a misaligned base, and the argument errors."""
import numpy as np
import pytest
import torch

import had_ref as hr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = {"f16": 1234.0, "bf16": 1232.0, "f32": 1234.5, "f64": 1234.25}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import gptq_svd_amd._lib as L
    return L


def image(x, pad, lead, sent):
    """x (rows, n) inside a flat sentinel buffer: `lead` elements in front, row
    stride n + pad.  Returns (buffer, view)."""
    rows, n = x.shape
    ld = n + pad
    buf = torch.full((lead + rows * ld,), sent, dtype=x.dtype, device=DEV)
    view = buf[lead:].view(rows, ld)[:, :n]
    view.copy_(x)
    return buf, view


def sentinels_intact(buf, rows, n, pad, lead, sent):
    body = buf[lead:].view(rows, n + pad)[:, n:]
    return bool((buf[:lead] == sent).all()) and bool((body == sent).all())


def run(L, xv, b, words, inverse, yv):
    n = xv.shape[1]
    w = None if words is None else torch.from_numpy(words).to(DEV)
    L.call("tg_hadamard", L.stream(), L.ptr(xv), L.DTYPES[xv.dtype], xv.shape[0], n, xv.stride(0),
           b, L.ptr(w), int(inverse), L.ptr(yv), L.DTYPES[yv.dtype], yv.stride(0))
    torch.cuda.synchronize()


def same_bits(a, b):
    return np.array_equal(hr.raw_bits(a), hr.raw_bits(b))


def random_rows(rows, n, dt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, n, generator=g, dtype=torch.float64) * 3.0
    return x.to(hr.TDT[dt])


@pytest.mark.parametrize("b", hr.BLOCKS)
def test_rows_bit_equal_over_shapes_and_types(L, b):
    """Every (n, rows) x every type pair, mixed signs, contiguous."""
    for n in (b, 3 * b):
        words = hr.pack_signs(hr.mixed_signs(n, b, b))
        for rows in hr.ROWS:
            ref, xs = {}, {}
            for xdt, ydt in hr.DTYPE_PAIRS:
                if xdt not in xs:
                    xs[xdt] = random_rows(rows, n, xdt, rows + n)
                    ct = "f64" if xdt == "f64" else "f32"
                    ref[xdt] = hr.rows(xs[xdt], b, words, out=ct)
                x = xs[xdt].to(DEV)
                y = torch.empty((rows, n), dtype=hr.TDT[ydt], device=DEV)
                run(L, x, b, words, False, y)
                assert same_bits(y, ref[xdt].to(hr.TDT[ydt])), (n, rows, xdt, ydt)


@pytest.mark.parametrize("b", hr.BLOCKS)
def test_rows_integer_data_is_exact(L, b):
    """|x| <= 8 integers against the explicit Sylvester product (f32 and f64
    outputs: every sum is exact, the multiply by c is the one rounding)."""
    Hb = hr.sylvester(b)
    for n, rows in ((b, 3), (3 * b, 17)):
        s = hr.mixed_signs(n, b, 1)
        words = hr.pack_signs(s)
        x = hr.integer_rows(rows, n, n)
        unscaled = ((x * s).reshape(rows, n // b, b) @ Hb).reshape(rows, n)
        inv = (x.reshape(rows, n // b, b) @ Hb).reshape(rows, n) * s
        for xdt, ydt, ct in (("f16", "f32", np.float32), ("f64", "f64", np.float64)):
            xd = torch.from_numpy(x).to(hr.TDT[xdt]).to(DEV)
            y = torch.empty((rows, n), dtype=hr.TDT[ydt], device=DEV)
            run(L, xd, b, words, False, y)
            assert np.array_equal(y.cpu().numpy(), unscaled.astype(ct) * hr.scale_of(b, ct))
            run(L, xd, b, words, True, y)
            assert np.array_equal(y.cpu().numpy(), inv.astype(ct) * hr.scale_of(b, ct))


@pytest.mark.parametrize("b", hr.BLOCKS)
def test_rows_signs_inverse_in_place_and_repeat(L, b):
    n, rows = 3 * b, 17
    words = hr.pack_signs(hr.mixed_signs(n, b, 2))
    for xdt in ("f16", "bf16", "f32", "f64"):
        x = random_rows(rows, n, xdt, b)
        xd = x.to(DEV)
        for w in (None, words):
            for inverse in (False, True):
                want = hr.rows(x, b, w, inverse=inverse)
                y = torch.empty_like(xd)
                run(L, xd, b, w, inverse, y)
                assert same_bits(y, want), (xdt, w is None, inverse)
                y2 = torch.empty_like(xd)
                run(L, xd, b, w, inverse, y2)
                assert same_bits(y, y2)                      # two calls bit-identical
                z = xd.clone()
                run(L, z, b, w, inverse, z)                  # in place
                assert same_bits(z, want), (xdt, w is None, inverse, "in place")
    # R^-1 R = identity bit for bit on integer data when c is a power of two
    if int(np.log2(b)) % 2 == 0:
        xi = torch.from_numpy(hr.integer_rows(rows, n, 3)).float().to(DEV)
        y = torch.empty_like(xi)
        run(L, xi, b, words, False, y)
        run(L, y, b, words, True, y)
        assert torch.equal(y, xi)


@pytest.mark.parametrize("b", [32, 128, 512, 1024, 4096])
@pytest.mark.parametrize("lay", ["pad_vec", "pad_odd", "misaligned"])
def test_rows_strided_views_keep_their_sentinels(L, b, lay):
    """pad_vec: strides that keep 16-byte accesses; pad_odd: strides that do not;
    misaligned: a base pointer one element off (the scalar path)."""
    n, rows = 3 * b, 3
    words = hr.pack_signs(hr.mixed_signs(n, b, 4))
    for xdt, ydt in (("f16", "f16"), ("bf16", "f32"), ("f32", "bf16"), ("f64", "f64")):
        per16 = 16 // torch.empty(0, dtype=hr.TDT[xdt]).element_size()
        per16y = 16 // torch.empty(0, dtype=hr.TDT[ydt]).element_size()
        xpad, ypad, lead = {"pad_vec": (per16, 2 * per16y, 0), "pad_odd": (3, 5, 0),
                            "misaligned": (0, 0, 1)}[lay]
        x = random_rows(rows, n, xdt, b + 1)
        want = hr.rows(x, b, words, out=ydt)
        xbuf, xv = image(x.to(DEV), xpad, lead, SENT[xdt])
        ybuf, yv = image(torch.zeros(rows, n, dtype=hr.TDT[ydt], device=DEV), ypad, lead, SENT[ydt])
        run(L, xv, b, words, False, yv)
        assert same_bits(yv, want), (xdt, ydt)
        assert sentinels_intact(ybuf, rows, n, ypad, lead, SENT[ydt])
        assert sentinels_intact(xbuf, rows, n, xpad, lead, SENT[xdt]) and same_bits(xv, x)
        if xdt == ydt:                                        # in place inside the image
            run(L, xv, b, words, False, xv)
            assert same_bits(xv, want)
            assert sentinels_intact(xbuf, rows, n, xpad, lead, SENT[xdt])


@pytest.mark.parametrize("n,b", hr.SYM_CASES)
def test_sym_bit_equal_and_symmetric(L, n, b):
    from mx_ref import hessian_case
    rng = np.random.default_rng(n + b)
    H = hessian_case(n, 2 * n, 1) if n <= 768 else None
    if H is None:                     # a cheap dense symmetric matrix at 4096
        A = rng.standard_normal((n, 64))
        H = A @ A.T / 64 + np.diag(np.exp(rng.standard_normal(n)))
    words = hr.pack_signs(hr.mixed_signs(n, b, 5))
    want = hr.sym(H, b, words)
    for pad in (0, 3):
        buf, Hv = image(torch.from_numpy(H), pad, 0, SENT["f64"])
        w = torch.from_numpy(words).to(DEV)
        L.call("tg_hadamard_sym", L.stream(), L.ptr(Hv), n, Hv.stride(0), b, L.ptr(w))
        torch.cuda.synchronize()
        got = Hv.contiguous().cpu().numpy()
        assert np.array_equal(got, got.T)
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), pad
        assert sentinels_intact(buf, n, n, pad, 0, SENT["f64"])
    if n <= 768:                      # null signs
        Hd = torch.from_numpy(H).to(DEV)
        L.call("tg_hadamard_sym", L.stream(), L.ptr(Hd), n, n, b, None)
        torch.cuda.synchronize()
        assert np.array_equal(Hd.cpu().numpy(), hr.sym(H, b, None))


def test_argument_errors(L):
    x = torch.zeros(2, 96, dtype=torch.float32, device=DEV)
    y = torch.zeros(2, 96, dtype=torch.float32, device=DEV)
    y64 = torch.zeros(2, 96, dtype=torch.float64, device=DEV)
    f = L.lib.tg_hadamard
    S, P, D = L.stream, L.ptr, L.DTYPES

    def rc(xx, n, ldx, b, yy, ldy, rows=2):
        return f(S(), P(xx), D[xx.dtype], rows, n, ldx, b, None, 0, P(yy), D[yy.dtype], ldy)

    assert rc(x, 96, 96, 48, y, 96) == -7 and "power of two" in L.last_error()   # not a power of two
    assert rc(x, 96, 96, 64, y, 96) == -7 and "divide" in L.last_error()         # b does not divide n
    assert rc(x, 96, 96, 16, y, 96) == -7                                        # b < 32
    assert rc(x, 96, 96, 8192, y, 96) == -7
    assert rc(x, 96, 96, 32, y64, 96) == -11 and "TG_F64" in L.last_error()      # f64 out of f32 in
    assert rc(y64, 96, 96, 32, y, 96) == -11
    assert rc(x, 96, 95, 32, y, 96) == -6
    assert rc(x, 96, 96, 32, y, 95) == -12
    assert rc(x, 96, 96, 32, y, 96, rows=0) == -4
    assert f(S(), None, 2, 2, 96, 96, 32, None, 0, P(y), 2, 96) == -2
    assert f(S(), P(x), 7, 2, 96, 96, 32, None, 0, P(y), 2, 96) == -3
    # in place with another stride
    assert f(S(), P(x), 2, 1, 64, 96, 32, None, 0, P(x), 2, 64) == -10
    g = L.lib.tg_hadamard_sym
    H = torch.zeros(96, 96, dtype=torch.float64, device=DEV)
    assert g(S(), P(H), 96, 96, 64, None) == -5
    assert g(S(), P(H), 96, 96, 48, None) == -5
    assert g(S(), P(H), 96, 95, 32, None) == -4
    assert g(S(), None, 96, 96, 32, None) == -2
    assert rc(x, 96, 96, 32, y, 96) == 0 and g(S(), P(H), 96, 96, 32, None) == 0
    torch.cuda.synchronize()
