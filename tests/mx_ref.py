"""Host reference of the MXFP4 weight format (A15) for test_gpu_mx.py; proved
on the CPU in test_mx_ref.py.  Plain numpy restatement of the contract in
include/truncgptq.h: every fp32 operation is one numpy float32 operation in the
order the contract writes it.

  group_scales      a = max |w| per 32 columns -> (2^E f32, byte E + 127)
  quantize_elements the seven compares; division, or the multiply by 2^-E
  decode            float(+-grid[code & 7]) * 2^(byte - 127), one rounding
  gptq_fwrd_mx      the block loop (loop=False), the comparator loop
                    (loop=True), the cross-block fmaf chain and the tail of
                    oracle.gptq_fwrd with the element rule swapped in
  rtn               plain MX casting of a weight matrix (no error feedback)
  pack              qweight (oracle.pack_rows_bitstream) and the transposed bytes
"""
import numpy as np
import torch

F32 = np.float32
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=F32)
MXG = 32
EMAX = 2            # E2M1's largest exponent: 6 = 1.5 * 2^2
TDT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def oracle():
    from oracle import oracle as o
    return o


def scale_exponent(a):
    """E = max(floor(log2 a) - 2, -126) for a >= 0 (float32; subnormals by their
    true floor(log2), a == 0 as -inf)."""
    a = np.asarray(a, dtype=F32)
    assert np.all(np.isfinite(a)) and np.all(a >= 0)
    _, ex = np.frexp(a)                       # a = f 2^ex, f in [0.5, 1): floor(log2 a) = ex - 1
    e = ex.astype(np.int64) - 1
    e = np.where(a == 0, np.int64(-10 ** 6), e)
    return np.maximum(e - EMAX, -126)


def pow2(E):
    """2^E as float32 (exact, subnormals included)."""
    return np.ldexp(F32(1.0), np.asarray(E).astype(np.int32)).astype(F32)


def group_scales(W):
    """W (m, n) -> scale (m, n/32) float32 = 2^E, byte (m, n/32) uint8 = E + 127."""
    W = np.asarray(W, dtype=F32)
    m, n = W.shape
    assert n % MXG == 0
    a = np.max(np.abs(W.reshape(m, n // MXG, MXG)), axis=2)
    E = scale_exponent(a)
    assert E.min() >= -126 and E.max() <= 125
    return pow2(E), (E + 127).astype(np.uint8)


def quantize_elements(w, scale, recip=False):
    """-> (qv float32, code uint8).  recip: t = w * (1 / scale) instead of
    w / scale (1 / scale is exact for a normal power of two)."""
    w = np.asarray(w, dtype=F32)
    scale = np.asarray(scale, dtype=F32)
    t = (w * (F32(1.0) / scale)).astype(F32) if recip else (w / scale).astype(F32)
    a = np.abs(t)
    idx = ((a > F32(0.25)).astype(np.int64) + (a >= F32(0.75)) + (a > F32(1.25))
           + (a >= F32(1.75)) + (a > F32(2.5)) + (a >= F32(3.5)) + (a > F32(5.0)))
    neg = (t < 0) & (idx != 0)
    q = (GRID[idx] * scale).astype(F32)
    qv = np.where(neg, -q, q).astype(F32)
    code = (idx | np.where(neg, 8, 0)).astype(np.uint8)
    return qv, code


def decode32(code, byte):
    """float32 decode: float(+-grid[code & 7]) * ldexpf(1, byte - 127)."""
    code = np.asarray(code).astype(np.int64)
    g = GRID[code & 7]
    g = np.where(code & 8, -g, g).astype(F32)
    s = pow2(np.asarray(byte).astype(np.int64) - 127)
    with np.errstate(over="ignore"):          # 4 and 6 overflow from byte 253 up
        return (g * s).astype(F32)


def decode(code, byte, out="f32"):
    """The decode rounded once (nearest even) to `out`: a CPU torch tensor."""
    return torch.from_numpy(np.ascontiguousarray(decode32(code, byte))).to(TDT[out])


def expand(scale):
    return np.repeat(scale, MXG, axis=1)


def rtn(W):
    """Plain MX casting: -> (Wq float32, codes uint8, scale, byte)."""
    W = np.asarray(W, dtype=F32)
    scale, byte = group_scales(W)
    qv, code = quantize_elements(W, expand(scale))
    return qv, code, scale, byte


def process_block_mx(w, s, R, loop):
    """oracle.process_block (loop=False) / process_block_loop (loop=True) with
    the E2M1 element rule.  -> (q, e, codes)."""
    w = np.array(w, dtype=F32, copy=True)
    s = np.asarray(s, dtype=F32)
    R = np.asarray(R, dtype=F32)
    m, B = w.shape
    q = np.empty_like(w)
    e = np.empty_like(w)
    codes = np.empty((m, B), dtype=np.uint8)
    for c in range(B):
        wc = w[:, c].copy()
        qv, code = quantize_elements(wc, s[:, c], recip=True)
        q[:, c] = qv
        codes[:, c] = code
        if loop:
            err = ((wc - qv) / R[c, c]).astype(F32)
            corr = R[c, c + 1:]
        else:
            err = (wc - qv).astype(F32)
            corr = (R[c, c + 1:] * (F32(1.0) / R[c, c])).astype(F32)
        e[:, c] = err
        w[:, c + 1:] = w[:, c + 1:] - (err[:, None] * corr[None, :]).astype(F32)
    return q, e, codes


def gptq_fwrd_mx(W, U, perm, block_size=1024, loop=False):
    """oracle.gptq_fwrd (gemm="fma") on the E2M1 grid.  W (m, n), U (k, n),
    perm (n,).  -> (Wq float32, codes uint8, both in the original column order,
    scale (m, n/32) float32, byte (m, n/32) uint8)."""
    W = np.asarray(W, dtype=F32)
    m, n = W.shape
    U32 = np.asarray(U, dtype=F32)
    k = U32.shape[0]
    perm = np.asarray(perm, dtype=np.int64)
    scale, byte = group_scales(W)
    Wp = np.ascontiguousarray(W[:, perm])
    S = np.ascontiguousarray(expand(scale)[:, perm])
    Q = np.zeros_like(Wp)
    C = np.zeros((m, n), dtype=np.uint8)
    for i1 in range(0, k, block_size):
        i2 = min(i1 + block_size, k)
        qb, eb, cb = process_block_mx(Wp[:, i1:i2], S[:, i1:i2], U32[i1:i2, i1:i2], loop)
        Q[:, i1:i2] = qb
        C[:, i1:i2] = cb
        if i2 < n:
            if loop:
                sm = np.ascontiguousarray(U32[i1:i2, i2:])
            else:
                sm = (U32[i1:i2, i2:] / np.diagonal(U32[i1:i2, i1:i2])[:, None]).astype(F32)
            Wp[:, i2:] = Wp[:, i2:] - oracle().fma_chain_matmul(eb, sm)
    if k < n:
        Q[:, k:], C[:, k:] = quantize_elements(Wp[:, k:], S[:, k:])
    inv = np.argsort(perm)
    return Q[:, inv], C[:, inv], scale, byte


def pack(codes, byte):
    """-> (qweight int32 (n/8, m), scales uint8 (n/32, m))."""
    qweight = oracle().pack_rows_bitstream(np.asarray(codes).T, 4)
    return qweight, np.ascontiguousarray(np.asarray(byte, dtype=np.uint8).T)


def raw_bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).numpy()


# ---------------------------------------------------------------------------
# shared fixtures of the tests
# ---------------------------------------------------------------------------
TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]


def tie_points():
    """Every tie point, its two float32 neighbours, the grid values, beyond
    saturation, zero -- in both signs (float32, 2 * 33 values)."""
    v = []
    for t in TIES:
        t = F32(t)
        v += [np.nextafter(t, F32(0)), t, np.nextafter(t, F32(100))]
    v += [float(g) for g in GRID] + [6.5, 7.0, 100.0, 1e-3]
    v = np.array(v, dtype=F32)
    return np.concatenate([v, -v])


def hessian_case(n, rows, seed):
    """Seeded X^T X / rows (float64) of correlated rows."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((rows, n)) @ (np.eye(n) + 0.3 * rng.standard_normal((n, n)) / np.sqrt(n))
    X = X * np.exp(rng.standard_normal(n))[None, :]
    return (X.T @ X) / rows


def shape_one(seed=0):
    """The first quantise shape of the issue: m = 17, n = 160, U and perm from
    oracle.process_hessian_alt on a seeded X^T X, k forced to 112 by truncating
    U.  Column perm[0] (no update reaches it) holds every tie point times its
    group's scale in both signs (rows 0..13; rows 14..16 hold two neighbours of a
    tie and -0); another column of that group holds 5 (rows alternate in
    sign), which pins a into [4, 8): E = 0, scale 1.
    -> (W, U (k, n) float32, perm, the planted column, its values)."""
    m, n, k = 17, 160, 112
    f = oracle().process_hessian_alt(hessian_case(n, 4 * n, seed), 1e-6, "energy")
    assert f.k >= k
    rng = np.random.default_rng(seed + 1)
    W = (rng.standard_normal((m, n)) * 0.7).astype(F32)
    c0 = int(f.perm[0])
    g0 = c0 // MXG
    pin = g0 * MXG + ((c0 % MXG) + 1) % MXG
    W[:, g0 * MXG:(g0 + 1) * MXG] = np.clip(W[:, g0 * MXG:(g0 + 1) * MXG], -3.9, 3.9)
    W[:, pin] = np.where(np.arange(m) % 2 == 0, 5.0, -5.0).astype(F32)
    ties = np.array(TIES, dtype=F32)
    planted = np.concatenate([ties, -ties, [np.nextafter(F32(2.5), F32(9)),
                                            np.nextafter(F32(-3.5), F32(0)), F32(-0.0)]])
    assert planted.shape == (m,)
    W[:, c0] = planted.astype(F32)
    return W, f.U[:k].astype(F32), f.perm, c0, planted.astype(F32)


def exact_gemm_case(m, n, T, seed, distinct=False):
    """Exact integer data for the GEMM: E2M1 codes restricted to the integer
    grid values {0, 1, 2, 3, 4, 6} in both signs, X integers in [-2, 2], and
    scale byte 127 (scale 1) -- or, with distinct, byte 127 + (3 u + r) % 5 for
    unit u of row r (scales 1 .. 16, consecutive units always differ), so a
    stale scale shows.  Every product and every partial sum is an integer; the
    caller asserts abs_int < 2^24, below which fp32 holds them exactly in any
    order.
    -> dict(codes (m, n) uint8, byte (m, n/32) uint8, X (T, n) int64,
            w_int (m, n) int64, y_int (T, m) int64, abs_int (T, m) int64)."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(np.array([0, 2, 4, 5, 6, 7]), size=(m, n))
    neg = (rng.integers(0, 2, size=(m, n)) == 1) & (idx != 0)
    codes = (idx | np.where(neg, 8, 0)).astype(np.uint8)
    G = n // MXG
    byte = np.full((m, G), 127, dtype=np.uint8)
    if distinct:
        byte = (127 + (3 * np.arange(G)[None, :] + np.arange(m)[:, None]) % 5).astype(np.uint8)
    w = decode32(codes, expand(byte))
    w_int = np.rint(w).astype(np.int64)
    assert np.array_equal(w_int.astype(F32), w)
    X = rng.integers(-2, 3, size=(T, n))
    y_int = X @ w_int.T
    abs_int = np.abs(X) @ np.abs(w_int).T
    return dict(codes=codes, byte=byte, X=X, w_int=w_int, y_int=y_int, abs_int=abs_int)


def exact_bias(m, seed):
    """(m,) float32 integers in [-100, 100]: exact in fp16, bf16 and fp32."""
    return np.random.default_rng(seed).integers(-100, 101, size=m).astype(F32)
