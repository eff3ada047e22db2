"""Host reference of the MXFP8 activation format (A16) for test_gpu_mxa.py;
proved on the CPU in test_mxa_ref.py.  Plain numpy restatement of the contract
in include/truncgptq.h: every fp32 operation is one numpy float32 operation in
the order the contract writes it.

  scale_bytes    a = max |x| per 32 columns -> max(exponent_field(a) - 8, 0)
  round_e4m3     |t| -> the nearest e4m3fn magnitude, ties to even, subnormals
                 kept, saturating at 448 (float64 arithmetic, exact)
  encode_e4m3    a grid magnitude and a sign bit -> the OCP byte
  quantize       X (fp16 / bf16 tensor, or float32 array) -> (xq, xs)
  decode         (xq, xs) -> float32
  exact_x        the integer activations of the exact GEMM tests
  planted_blocks the blocks of 32 the quantiser tests plant

Sign rule: the sign bit of q is the sign bit of x, always (-0 and negative values
that round to zero give 0x80).
"""
import ctypes

import numpy as np
import torch

F32 = np.float32
BLK = 32
EMAX = 8            # e4m3's largest exponent: 448 = 1.75 * 2^8
SAT = 448.0
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}

# the split-K shape of test_gpu_mxa.py: the smallest n at which tg_qgemm_mx_act
# splits K (8 steps of 128: two splits of 4 steps); m as in the other GEMM tests
SPLIT_M, SPLIT_N = 104, 1024


def as_f32(X):
    """fp16 / bf16 tensor or array -> float32 array (exact)."""
    if isinstance(X, torch.Tensor):
        return X.detach().cpu().float().numpy()
    return np.asarray(X, dtype=F32)


def scale_bytes(a):
    """a >= 0 float32 -> max(exponent_field(a) - 8, 0) as uint8."""
    a = np.ascontiguousarray(a, dtype=F32)
    assert np.all(np.isfinite(a)) and np.all(a >= 0)
    ef = (a.view(np.uint32) >> 23).astype(np.int64)
    return np.maximum(ef - EMAX, 0).astype(np.uint8)


def pow2(E):
    return np.ldexp(F32(1.0), np.asarray(E).astype(np.int32)).astype(F32)


def round_e4m3(t):
    """|t| (any float) -> float64 magnitude on the e4m3fn grid."""
    a = np.abs(np.asarray(t, dtype=np.float64))
    _, ex = np.frexp(a)                         # a = f 2^ex, f in [0.5, 1)
    e = np.maximum(ex.astype(np.int64) - 1, -6)  # below 2^-6 the spacing stays 2^-9
    ulp = np.ldexp(1.0, (e - 3).astype(np.int32))
    q = np.rint(a / ulp) * ulp                  # exact: rint is ties-to-even
    return np.minimum(q, SAT)


def encode_e4m3(q, neg):
    """grid magnitude q (float64), sign bits -> uint8."""
    q = np.asarray(q, dtype=np.float64)
    f, ex = np.frexp(q)
    e = ex.astype(np.int64) - 1
    normal = (((e + 7) << 3) | np.rint((2 * f - 1) * 8).astype(np.int64))
    byte = np.where(q < 2.0 ** -6, np.rint(q * 512).astype(np.int64), normal)
    assert byte.min() >= 0 and byte.max() <= 0x7e
    return (byte | np.where(neg, 0x80, 0)).astype(np.uint8)


def quantize(X):
    """X (T, n) -> (xq (T, n) uint8 e4m3fn, xs (T, n/32) uint8 E8M0)."""
    x = as_f32(X)
    T, n = x.shape
    assert n % BLK == 0 and np.all(np.isfinite(x))
    xb = x.reshape(T, n // BLK, BLK)
    xs = scale_bytes(np.max(np.abs(xb), axis=2))
    up = pow2(127 - xs.astype(np.int64))        # 2^(127 - byte): 2^-119 .. 2^127, normal
    with np.errstate(under="ignore"):
        t = (xb * up[:, :, None]).astype(F32)
    assert np.all(np.abs(t) < 512)
    xq = encode_e4m3(round_e4m3(t), np.signbit(xb))
    return xq.reshape(T, n), xs


def decode_e4m3(b):
    """uint8 -> float32 (OCP e4m3fn; 0x7f / 0xff are NaN and never written)."""
    b = np.asarray(b).astype(np.int64)
    e, mant = (b >> 3) & 15, b & 7
    mag = np.where(e == 0, mant * 2.0 ** -9, (8 + mant) * np.ldexp(1.0, (e - 10).astype(np.int32)))
    return np.where(b & 0x80, -mag, mag).astype(F32)


def decode(xq, xs):
    """X^ (T, n) float32 = e4m3(xq) * 2^(xs - 127)."""
    s = pow2(np.asarray(xs).astype(np.int64) - 127)
    return (decode_e4m3(xq) * np.repeat(s, BLK, axis=1)).astype(F32)


def nextbelow(v, dt):
    """The largest value of dtype dt below v > 0 (float)."""
    t = torch.tensor([v], dtype=TDT[dt])
    return float((t.view(torch.int16) - 1).view(TDT[dt]).float())


def planted_blocks(dt):
    """[(name, 32 float32 values exact in dt)]: the scale and rounding cases of
    the contract.  Blocks named t128_* have max |x| = 2, hence byte 120 and
    t = 128 x, so their other entries are chosen in t."""
    rng = np.random.default_rng(7)
    out = []

    def block(name, a, rest, pos=5):
        v = np.array(rest, dtype=np.float64)
        v = np.concatenate([v, np.zeros(BLK - 1 - v.size)])
        v = np.insert(v, pos, a)
        out.append((name, torch.from_numpy(v).to(TDT[dt]).float().numpy()))
        assert np.array_equal(out[-1][1].astype(np.float64), v), name   # exact in dt

    small = (rng.integers(-64, 65, 31) / 64.0)
    block("pow2", 4.0, small * 2)
    block("below_pow2", -nextbelow(4.0, dt), small * 2, pos=31)
    block("saturate", 15.0, np.concatenate([[-15.0, 14.0, -14.0, 15.0], small[:27] * 8]), pos=0)
    block("zero", 0.0, [-0.0, 0.0, -0.0])
    if dt == "f16":
        block("f16_subnormal", 3 * 2.0 ** -24, [2.0 ** -24, -2.0 ** -23, 0.0, -(2.0 ** -24)])
    else:
        block("bf16_huge", -1.5 * 2.0 ** 120, small * 2.0 ** 119, pos=17)
        block("bf16_subnormal", 2.0 ** -130, [-(2.0 ** -131), 2.0 ** -133, -0.0])
    # ties in t = 128 x: 17 -> 16 and 19 -> 20 (spacing 2); 216 -> 224 (mantissa 110, even) and
    # 232 -> 224 (spacing 16); 17.5, 18.5, 16.5 are off the ties
    ties = [17, -17, 19, -19, 216, -216, 232, -232, 17.5, 18.5, 16.5, -16.5]
    # the subnormals, spacing 2^-9: ties 2^-10 -> 0, 3 2^-10 -> 2^-8, 7.5 2^-9 -> 2^-6 (normal);
    # 1.5 2^-10 -> 2^-9; 2^-6 (1 + 1/16) -> 2^-6; 0.9 2^-10-ish -> 0
    sub = [2.0 ** -10, -(2.0 ** -10), 3 * 2.0 ** -10, 7.5 * 2.0 ** -9, -7.5 * 2.0 ** -9,
           1.5 * 2.0 ** -10, 2.0 ** -6 * (1 + 1 / 16), 2.0 ** -6, 7 * 2.0 ** -9, 2.0 ** -11,
           -(2.0 ** -11), 2.0 ** -6 * (1 + 3 / 16)]
    block("t128_ties", 2.0, np.array(ties + sub) / 128.0, pos=9)
    block("large_and_tiny", 1000.0, np.concatenate([[-(2.0 ** -14), 2.0 ** -14, -0.0],
                                                    small[:28] * 2.0 ** -12]), pos=30)
    return out


def quant_case(T, n, dt, seed=0):
    """Random X (T, n) of dtype dt with as many planted blocks as fit, starting
    at a block offset that depends on the shape.  -> CPU tensor."""
    gen = torch.Generator().manual_seed(seed + 31 * T + n)
    x = (torch.randn(T, n, generator=gen) * torch.exp(2 * torch.randn(T, 1, generator=gen)))
    x = x.to(TDT[dt])
    pl = planted_blocks(dt)
    nb = T * (n // BLK)
    xb = x.reshape(nb, BLK)
    for i in range(min(nb, len(pl))):
        xb[i] = torch.from_numpy(pl[(i + T + n // BLK) % len(pl)][1]).to(TDT[dt])
    return xb.reshape(T, n)


def exact_x(T, n, seed):
    """(T, n) int64: integers in [-15, 15] times 2^((2 u + 3 r) % 4) for block u
    of row r, and in every block one entry of magnitude 16 (same factor).  The
    planted 16 pins the block's maximum into [16, 32) 2^p, so t = 16 x_int <= 256
    and every entry is a four-bit integer times a power of two: exact in e4m3.
    Without it a block whose largest entry is 15 (mantissa 1.875 > 1.75) would
    saturate to 14.  Neighbouring blocks and rows carry different scale bytes."""
    rng = np.random.default_rng(seed)
    G = n // BLK
    x = rng.integers(-15, 16, size=(T, G, BLK))
    r, u = np.arange(T)[:, None], np.arange(G)[None, :]
    pos = (5 * u + 3 * r) % BLK
    sign = np.where((u + r) % 2 == 0, 16, -16)
    np.put_along_axis(x, pos[:, :, None], sign[:, :, None], axis=2)
    x = x * (2 ** ((2 * u + 3 * r) % 4))[:, :, None]
    return x.reshape(T, n).astype(np.int64)


def act_workspace_split(lib, T, m, n):
    """(S, steps per split) of tg_qgemm_mx_act at (T, m, n), read from
    tg_qgemm_mx_act_workspace_size: X^ as 2048 + 64 bytes per (tile of 16 rows,
    K step of 128) (+ 255 of slack each) and, when S > 1, S T m floats (+ 255)."""
    lib.tg_qgemm_mx_act_workspace_size.restype = ctypes.c_size_t
    ws = int(lib.tg_qgemm_mx_act_workspace_size(T, m, n))
    steps = -(-n // 128)
    ts = -(-T // 16) * steps
    rest = ws - (ts * 2048 + 255) - (ts * 64 + 255)
    assert rest >= 0
    if rest == 0:
        return 1, steps
    assert (rest - 255) % (T * m * 4) == 0
    S = (rest - 255) // (T * m * 4)
    return S, -(-steps // S)
