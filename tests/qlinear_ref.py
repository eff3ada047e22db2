"""Host references and the shared case lists of the packed-inference tests
(test_gpu_qlinear.py, test_gpu_qlinear_edges.py; checked without a GPU in
test_qlinear_ref.py).

Helpers
  packed_case     random codes / zeros / scales packed by the oracle; any n and
                  g with n * b and m * b whole numbers of 32-bit words
  packed_fill     the two saturating patterns at scale 65504
  host_dequant    float32(code - zero) * float32(scale), one rounding
  exact_reference the GEMM on data where every product and every partial sum is
                  an exact fp32 value, so any summation order gives the same bits
  exact_case      the inputs and the expected output of one Case, computed once
                  per process and shared; callers leave the arrays unchanged

The exact reference: X holds integers (times a power of two in the "hot" rows),
the scales are 2^-6 .. 2^-2 and the bias entries are multiples of 2^-6, so with
y_int = 64 y every term of the sum is an integer.  While the sum of the
*absolute* terms (bias included) stays below 2^24, every partial sum of every
summation order is an integer below 2^24, hence exact in fp32, and the kernel
must reproduce y_int / 64 bit for bit.  For a 16-bit output the expected bits
are that fp32 value converted once by torch (round to nearest even, overflow to
inf).

Case lists: every list the GPU file parametrises lives here, so the CPU test
can prove for each case that the reference is exact (the comparison cannot be
vacuous) and that the shapes meant to reach the gemv kernel's wave loop still
do with the current dispatch constants.
"""
import collections
import functools

import numpy as np
import torch

BITS = [2, 3, 4, 8]
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def oracle():
    from oracle import oracle as o
    return o


def group_index(n, g):
    return np.arange(n) // (g if g > 0 else n)


@functools.lru_cache(maxsize=None)
def packed_case(m, n, g, b, scale_kind, seed=0):
    """Random codes / zeros / scales packed by the oracle.  Returns the host
    arrays (codes, zeros unsigned ints; scale (m, G) float32) and the packed
    numpy tensors.  n and g need not be multiples of 32 (n * b and m * b must
    be multiples of 32, g must divide n)."""
    rng = np.random.default_rng(1000 * b + m + n + seed)
    G = n // (g if g > 0 else n)
    codes = rng.integers(0, 2 ** b, size=(m, n))
    zero = rng.integers(0, 2 ** b, size=(m, G))
    if scale_kind == "pow2":
        scale = (2.0 ** rng.integers(-6, -1, size=(m, G))).astype(np.float32)
    elif scale_kind == "small":      # W^ ~ O(0.05)
        scale = (rng.uniform(0.05, 0.1, size=(m, G)) / 2 ** (b - 1)).astype(np.float32)
    else:
        scale = rng.uniform(1e-3, 2e-2, size=(m, G)).astype(np.float32)
    qw, qz, sc = oracle().pack_weights(codes, scale, zero.astype(np.float32), b, False)
    return codes, zero, scale, qw, qz, sc


@functools.lru_cache(maxsize=None)
def packed_fill(m, n, g, b, fill):
    """Saturating data at scale 65504 (the largest fp16): fill "max" is every
    code 2^b - 1 with zero 0 (w = +(2^b - 1) 65504), fill "min" every code 0
    with zero 2^b - 1 (w = -(2^b - 1) 65504)."""
    top = 2 ** b - 1
    G = n // (g if g > 0 else n)
    codes = np.full((m, n), top if fill == "max" else 0, dtype=np.int64)
    zero = np.full((m, G), 0 if fill == "max" else top, dtype=np.int64)
    scale = np.full((m, G), 65504.0, dtype=np.float32)
    qw, qz, sc = oracle().pack_weights(codes, scale, zero.astype(np.float32), b, False)
    return codes, zero, scale, qw, qz, sc


def host_dequant(codes, zero, scale, g, out):
    """float32(code - zero) * float32(scale), one rounding to `out`; returned
    as a CPU torch tensor of that dtype."""
    gi = group_index(codes.shape[1], g)
    with np.errstate(over="ignore"):
        w32 = (codes - zero[:, gi]).astype(np.float32) * scale.astype(np.float32)[:, gi]
    assert w32.dtype == np.float32
    return torch.from_numpy(w32).to(TDT[out])


def raw_bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


def ulp(y64, dt):
    """Spacing of `dt` at |y64| (fp16: 11-bit significand, subnormal spacing
    2^-24; bf16: 8-bit significand)."""
    a = np.abs(y64)
    e = np.floor(np.log2(np.maximum(a, 1e-300)))
    if dt == "f16":
        return 2.0 ** (np.maximum(e, -14) - 10)
    return 2.0 ** (np.maximum(e, -126) - 7)


def weight_int(codes, zero, scale, g):
    """64 w as int64: (code - zero) * (64 scale), scales 2^-6 .. 2^-2."""
    gi = group_index(codes.shape[1], g)
    s64 = np.rint(scale[:, gi] * 64).astype(np.int64)
    assert np.array_equal(s64.astype(np.float32), scale[:, gi] * np.float32(64))
    return (codes - zero[:, gi]).astype(np.int64) * s64


def exact_reference(X, codes, zero, scale, g, bias=None, out="f32", w_int=None):
    """-> (want, y_int, abs_int).  X integer-valued (T, n); scales powers of two
    2^-6 .. 2^-2; bias None or (m,) multiples of 2^-6.  y_int = 64 (X W^T +
    bias) as int64, abs_int the same sum over absolute terms.  want is
    y_int / 64 as fp32 converted once to `out` by torch (CPU tensor); it is the
    exact result while abs_int < 2^24 (the caller asserts that).

    The products run in float64 through BLAS: every operand is an integer and
    every partial sum is far below 2^53, so they are exact in any order."""
    if w_int is None:
        w_int = weight_int(codes, zero, scale, g)
    X = np.asarray(X)
    assert np.array_equal(np.rint(X), X)
    x64, w64 = X.astype(np.float64), np.asarray(w_int, dtype=np.float64)
    y = x64 @ w64.T
    a = np.abs(x64) @ np.abs(w64).T
    if bias is not None:
        b64 = np.asarray(bias, dtype=np.float64) * 64
        assert np.array_equal(np.rint(b64), b64), "bias entries must be multiples of 2^-6"
        y = y + b64[None, :]
        a = a + np.abs(b64)[None, :]
    assert a.max() < 2.0 ** 53
    y_int, abs_int = np.rint(y).astype(np.int64), np.rint(a).astype(np.int64)
    want32 = (y_int.astype(np.float64) / 64).astype(np.float32)
    return torch.from_numpy(want32).to(TDT[out]), y_int, abs_int


# ---------------------------------------------------------------------------
# the cases of test_gpu_qlinear_edges.py
# ---------------------------------------------------------------------------
# xlay: where X lies.  "odd": aligned base, ldx = n + 5 (scalar loads in the
# mfma kernel); "vec": aligned base, ldx = n + 8 (16-byte loads); "off1": base
# one element past a 16-byte boundary, ldx = n + 8 (ldx % 8 == 0 but scalar
# loads all the same).
# hot: two rows of X are +-c sign(w[r0, :]) with c the largest power of two that
# keeps abs_int < 2^24, so y[0, r0] = -y[1, r0] is above fp16's 65504.
Case = collections.namedtuple("Case", "m n g b T xdt ydt bias xlay hot")

XLAY = {"odd": (0, 5), "vec": (0, 8), "off1": (1, 8)}   # (lead elements, ldx - n)
Y_LEAD, Y_PAD, TAIL = 1, 5, 7
SENT_X, SENT_Y = 3.0, -12288.0                          # exact in f16, bf16 and f32


def case(m, n, g, b, T, xdt, ydt="f32", bias=None, xlay=None, hot=False):
    if xlay is None:
        xlay = "vec" if T % 2 == 0 else "odd"
    return Case(m, n, g, b, T, xdt, ydt, bias, xlay, hot)


def regimes(T):
    return ["gemv", "mfma"] if T <= 16 else ["mfma"]


XDTS = ("f16", "bf16")

# (a) the production dispatch of the gemv regime at the smallest size that
# reaches it: some wave of a workgroup owns more than one unit of 32 values.
# m = 4416 (69 tiles of 64 features), n = 2048 (64 units): 15 splits wanted,
# 5 units per workgroup, 13 splits; waves 0 and 1 take two units, the last
# split has 4 units (one per wave).
WAVE_M, WAVE_N = 4416, 2048
# b = 8: m = 2240 (35 tiles), n = 4096 (128 units): 5 units per workgroup, 26 splits
WAVE8_M, WAVE8_N = 2240, 4096
# three units per wave: more than 8 units per workgroup needs at most 7 splits
# of the 64 units, i.e. cdiv(1024, tiles) <= 7, tiles >= 147: m > 146 * 64 = 9344;
# the smallest legal m (m * 4 % 32 == 0) is 9352 -- 10 units per workgroup,
# 7 splits, waves 0..2 take three units, the last tile has 8 features
WAVE3_M, WAVE3_B = 9352, 4
WAVE_SHAPES = [(WAVE_M, WAVE_N, 128, 3), (WAVE_M, WAVE_N, 128, 4), (WAVE_M, WAVE_N, 512, 3),
               (WAVE_M, WAVE_N, 512, 4), (WAVE8_M, WAVE8_N, 128, 8),
               (WAVE3_M, WAVE_N, 128, WAVE3_B)]
CASES_WAVE = [case(WAVE_M, WAVE_N, g, b, T, xdt)
              for g in (128, 512) for b in (3, 4) for T in (1, 4, 16) for xdt in XDTS]
CASES_WAVE += [case(WAVE8_M, WAVE8_N, 128, 8, 3, "f16")]
CASES_WAVE += [case(WAVE3_M, WAVE_N, 128, WAVE3_B, T, xdt) for T, xdt in ((1, "f16"), (4, "bf16"))]

# (b) group geometry: a group boundary inside a 128-value slab (g = 96), g = 64,
# a group spanning two slabs (g = 256), per-channel (g = n)
CASES_GROUP = [case(96, n, g, b, T, xdt)
               for n, g in ((192, 96), (384, 96), (256, 64), (512, 256), (512, -1), (96, -1))
               for b in BITS for T in (3, 40) for xdt in XDTS]

# (c) K tails: less than one slab, and a one- / three-unit tail after a full slab
CASES_KTAIL = [case(64, n, 32, b, T, xdt)
               for n in (32, 64, 160, 224) for b in BITS for T in (2, 20) for xdt in XDTS]

# (d) the smallest legal m of each width, one tile plus the smallest step, two
# tiles; n = g = 128
CASES_FEAT = [case(m, 128, 128, b, T, xdt)
              for b, m in ((8, 4), (4, 8), (2, 16), (3, 32), (8, 68), (4, 72), (2, 80), (3, 96),
                           (2, 128), (3, 128), (4, 128), (8, 128))
              for T, xdt in ((1, "f16"), (5, "bf16"), (70, "f16"))]

# (e) row buckets: the gemv kernel's TT = 2, 4, 8, 16 and their boundaries; both
# sides of the mfma regime's 64- / 128-row tile choice
CASES_ROWS = [case(96, 256, 128, 4, T, xdt)
              for T in (2, 4, 5, 8, 9, 15, 64, 65, 128, 129, 193) for xdt in XDTS]

# (f) X addressing
CASES_XADDR = [case(96, 256, 128, b, T, xdt, xlay=xlay)
               for b in (3, 4) for xdt in XDTS
               for T, xlay in ((3, "off1"), (16, "off1"), (3, "vec"), (1, "vec"), (1, "off1"),
                               (40, "off1"))]

# (g) outputs: 16-bit Y against the single rounding of the exact value, every
# bias type on each finishing path (gemv reduce; mfma writing Y itself, n = 256;
# mfma through the partials, n = 1024)
CASES_OUT = [case(96, n, 128, 4, T, dt, ydt=dt, bias=bias, hot=True)
             for n in (256, 1024) for T in (3, 70) for dt in XDTS
             for bias in (None, "f16", "bf16", "f32")]
CASES_OUT += [case(96, n, 128, 3, 3, dt, ydt="f32", bias=bias)
              for n in (256, 1024) for dt in XDTS for bias in ("f16", "bf16", "f32")]

EXACT_CASES = (CASES_WAVE + CASES_GROUP + CASES_KTAIL + CASES_FEAT + CASES_ROWS + CASES_XADDR
               + CASES_OUT)

# (j) dequant through the C ABI: short last unit / group switch inside a unit,
# then m > 256 (a second workgroup along the features)
DEQUANT_SHAPES = [(8, 40, 8, 4), (4, 36, 12, 8), (16, 48, 16, 2), (32, 96, 48, 3),
                  (288, 64, 32, 3), (264, 64, 64, 4), (260, 32, -1, 8), (272, 64, 32, 2)]
DEQUANT_FILL_SHAPES = DEQUANT_SHAPES[:4]

# (k) the project's own packers: the wave-loop shape (m > 256 in one kernel,
# 414 or 552 zero words per group in the other) and the short-unit shape
PACK_SHAPES = [(WAVE_M, WAVE_N, 128, 3), (WAVE_M, WAVE_N, 128, 4), (8, 40, 8, 4)]


@functools.lru_cache(maxsize=None)
def weight_int16(m, n, g, b):
    """weight_int of packed_case(m, n, g, b, "pow2"), kept small (|.| <= 255 * 16)."""
    codes, zero, scale, *_ = packed_case(m, n, g, b, "pow2")
    w = weight_int(codes, zero, scale, g)
    assert np.abs(w).max() < 2 ** 15
    w = w.astype(np.int16)
    w.setflags(write=False)
    return w


def exact_bias(c):
    """(m,) float32 multiples of 2^-6 in [-200, 200] / 64: at most 8 significant
    bits, so fp16, bf16 and fp32 all hold them exactly."""
    if c.bias is None:
        return None
    rng = np.random.default_rng(7 * c.m + c.n)
    bias = (rng.integers(-200, 201, size=c.m) / 64.0).astype(np.float32)
    t = torch.from_numpy(bias)
    assert torch.equal(t.to(TDT[c.bias]).float(), t)
    return bias


@functools.lru_cache(maxsize=None)
def exact_case(c):
    """-> dict(X int64 (T, n), bias float32 (m,) or None, want CPU tensor of
    c.ydt, y_int, abs_int)."""
    w_int = weight_int16(c.m, c.n, c.g, c.b).astype(np.int64)
    rng = np.random.default_rng(c.T * 31 + c.b)
    X = rng.integers(-2, 3, size=(c.T, c.n))
    bias = exact_bias(c)
    if c.hot:
        assert c.T >= 2
        rowsum = np.abs(w_int).sum(axis=1)
        r0 = int(np.argmax(rowsum))
        # the other rows of X add at most 2 * rowsum; the bias at most 200
        cmul = 2 ** int(np.floor(np.log2((2 ** 24 - 201) / rowsum[r0])))
        if cmul * rowsum[r0] + 200 >= 2 ** 24:
            cmul //= 2
        X[0] = cmul * np.sign(w_int[r0])
        X[1] = -X[0]
    codes, zero, scale, *_ = packed_case(c.m, c.n, c.g, c.b, "pow2")
    want, y_int, abs_int = exact_reference(X, codes, zero, scale, c.g, bias=bias, out=c.ydt,
                                           w_int=w_int)
    xt = torch.from_numpy(X).to(TDT[c.xdt])
    assert np.array_equal(xt.double().numpy(), X), "X is not exact in its dtype"
    for a in (X, y_int, abs_int) + (() if bias is None else (bias,)):
        a.setflags(write=False)
    return dict(X=X, bias=bias, want=want, y_int=y_int, abs_int=abs_int)


def x_image(c, X):
    """(flat CPU tensor of c.xdt, lead, ldx): X inside a sentinel-filled buffer."""
    lead, pad = XLAY[c.xlay]
    ldx = c.n + pad
    flat = torch.full((lead + c.T * ldx + TAIL,), SENT_X, dtype=TDT[c.xdt])
    xt = torch.from_numpy(np.array(X)).to(TDT[c.xdt])           # a copy: X is read-only
    flat[lead:lead + c.T * ldx].view(c.T, ldx)[:, :c.n] = xt
    return flat, lead, ldx


def y_image(T, m, dt, want=None):
    """(flat CPU tensor of dt, lead, ldy): the sentinel-filled output buffer, with
    `want` (T, m) in its place when given -- the whole expected image."""
    ldy = m + Y_PAD
    flat = torch.full((Y_LEAD + T * ldy + TAIL,), SENT_Y, dtype=TDT[dt])
    if want is not None:
        flat[Y_LEAD:Y_LEAD + T * ldy].view(T, ldy)[:, :m] = want
    return flat, Y_LEAD, ldy
