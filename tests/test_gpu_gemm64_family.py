"""The whole FP64 MFMA GEMM family of gemm64.hip, entry point by entry point,
through the test hooks tg_gemm64_probe / tg_gemm64_chunked: dgemm,
dgemm_upper_a, dgemm_splitk, sum_partials, the four SYRKs and dgemm_chunked
(tri = 0, 1, 2), at the smallest shapes that reach every kernel instantiation
and every edge of its staging, tile map and K-cut ("Which test
reaches which FP64 GEMM kernel").

Every operand sits in a padded, offset buffer (abi_helpers; layouts C, A, B and
the local V: aligned base, even ld > width, so an odd width ends in a ragged
16-byte pair).  Two references (gemm64_refs.py, self-tested on the CPU in
test_gemm64_refs.py):

  exact    integers in [-3, 3], alpha in {0.5, -2}, beta in {0, 1, -0.25}, C0
           integers in [-8, 8]: every intermediate is an exact double, so the
           result must equal numpy's int64 computation bit for bit;
  bounded  standard-normal data: |C - C_ref| <= 2 (K + 3) 2^-53 (|alpha| |op A|
           |op B| + |beta| |C0|) per element, derived (first-order any-order
           bound of a K-term FP64 dot product plus the alpha / beta roundings,
           twice because numpy's reference is an FP64 sum too), not measured;
           the worst err / bound is printed; two calls give identical bits.

In every case the columns N .. ldc-1, the lead-in and the tail of C still hold
the sentinel and A and B are bit-unchanged.  With beta == 0 the logical C is
prefilled with NaN and the result must be finite and equal.

Triangular operands (dgemm_upper_a, tri = 1 / 2): the zero triangle is skipped
per *tile* -- the K range of a tile row starts at the tile's first row (tm is
a multiple of the tile size), so the zeros inside the tile-sized diagonal
blocks are read and multiplied.  They hold zeros; everything strictly below
the diagonal blocks of the tile size in force holds NaN, which must not reach
C (gemm64_refs.tri_nan).
"""
import ctypes

import numpy as np
import pytest
import torch

import gemm64_refs as R
from abi_helpers import SENTINEL, logical, outside_intact, padded

pytestmark = pytest.mark.gpu

GEMM, UPPER_A, SPLITK, SUM_PARTIALS, SYRK_TN, SYRK_TN_UPPER, SYRK_TN_LOWER, SYRK_NT = range(8)
# (alpha, beta) of the exact cases: each alpha with each beta
AB = [(0.5, 0.0), (-2.0, 1.0), (0.5, -0.25), (-2.0, 0.0), (0.5, 1.0), (-2.0, -0.25)]
# layouts of (A, B, C): all-C, all-A, all-B, all-V, and V for A / B with B for C
LAYS = [("C", "C", "C"), ("A", "A", "A"), ("B", "B", "B"), ("V", "V", "V"), ("V", "V", "B")]
# one operand on the 16-byte path, the other not (the 8-wave kernel's VA / VB instances)
LAYS_MIXED = [("V", "B", "C"), ("B", "V", "C")]
TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]


@pytest.fixture(scope="module")
def L():
    from gptq_svd_amd import _lib
    return _lib


class Dev:
    """A host matrix in a padded device buffer (abi_helpers.padded) in `layout`."""

    def __init__(self, a, layout):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.shape = a.shape
        self.lead, self.ld = R.place(a.shape[1], layout)
        self.p, self.buf = padded(a, self.ld, self.lead)
        self.before = self.buf.clone()
        self.vec = self.p.value % 16 == 0 and self.ld % 2 == 0   # gemm64.hip vec_ok
        if layout == "V":
            assert self.p.value % 16 == 0 and self.ld % 2 == 0

    def at(self, off):
        return ctypes.c_void_p(self.p.value + 8 * off)

    def get(self):
        return logical(self.buf, self.shape, self.ld, self.lead)

    def flat(self):
        return self.buf.cpu().numpy()

    def intact(self):
        return outside_intact(self.buf, self.shape, self.ld, self.lead)

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int64), self.before.view(torch.int64))


def ints(rng, shape, lim=3):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)


def c_init(C0, beta):
    """What the logical C holds before the call: NaN when it must not be read."""
    return C0 if beta != 0.0 else np.full(C0.shape, np.nan)


def probe(L, op, ta, tb, M, N, K, alpha, A, B, beta, C, splits=1, ws=None):
    L.call("tg_gemm64_probe", L.stream(), op, ta, tb, M, N, K, alpha, A.p, A.ld,
           B.p if B is not None else None, B.ld if B is not None else 0, beta, C.p, C.ld, splits,
           L.ptr(ws), 0 if ws is None else ws.numel() * ws.element_size())


def gemm_case(L, op, ta, tb, M, N, K, alpha, beta, lays, rng, exact, splits=1, tile=None,
              entry="probe", seen=None):
    """One call of a GEMM-shaped op checked against its reference; returns the
    worst err / bound (0 for an exact case).  tile: A is upper triangular,
    poisoned below the diagonal blocks of that size (UPPER_A)."""
    gen = ints if exact else (lambda r, s, lim=None: r.standard_normal(s))
    Ah = gen(rng, (K, M) if ta else (M, K))
    Bh = gen(rng, (N, K) if tb else (K, N))
    C0 = gen(rng, (M, N), 8)
    Aref = Ah
    if tile is not None:
        Aref, Ah = np.triu(Ah), R.tri_nan(Ah, tile)
    A, B = Dev(Ah, lays[0]), Dev(Bh, lays[1])
    if seen is not None:
        seen.add((A.vec, B.vec))
    ws = None
    if op == SPLITK:
        nbytes = L.lib.tg_gemm64_probe_workspace_size(op, M, N, splits)
        assert nbytes == 8 * M * N * splits
        ws = torch.full((max(nbytes // 8, 1),), float("nan"), dtype=torch.float64, device="cuda:0")
    if exact:
        ref, bound = R.gemm_exact(ta, tb, alpha, Aref, Bh, beta, C0), None
    else:
        ref, bound = R.gemm_bound(ta, tb, alpha, Aref, Bh, beta, C0)
    outs = []
    for _ in range(1 if exact else 2):
        C = Dev(c_init(C0, beta), lays[2])
        if entry == "tg_dgemm":
            L.call("tg_dgemm", L.stream(), ta, tb, M, N, K, alpha, A.p, A.ld, B.p, B.ld, beta, C.p,
                   C.ld)
        else:
            probe(L, op, ta, tb, M, N, K, alpha, A, B, beta, C, splits, ws)
        got = C.get()
        what = (op, ta, tb, M, N, K, alpha, beta, lays, splits)
        assert C.intact(), f"wrote outside the logical C: {what}"
        assert A.unchanged() and B.unchanged(), f"an input changed: {what}"
        assert np.all(np.isfinite(got)), f"non-finite result: {what}"
        outs.append(got)
    if exact:
        assert np.array_equal(outs[0], ref), f"{what}: {R.first_mismatch(outs[0], ref)}"
        return 0.0
    assert np.array_equal(outs[0], outs[1]), f"two calls differ: {what}"
    ratio = R.worst_ratio(outs[0], ref, bound)
    assert ratio <= 1.0, f"err/bound {ratio:.3f}: {what}"
    return ratio


# ---- dgemm -------------------------------------------------------------------
KERNELS = {
    "tile64": {"TG_GEMM_TILE": "64"},
    "tile128x64": {"TG_GEMM_TILE": "12864"},
    "tile128-own": {"TG_GEMM_TILE": "128", "TG_GEMM_IMPL": "own"},
    "tile128-own8-swz": {"TG_GEMM_TILE": "128", "TG_GEMM_IMPL": "own8", "TG_GEMM_SWZ": "1"},
    "tile128-own8-2d": {"TG_GEMM_TILE": "128", "TG_GEMM_IMPL": "own8", "TG_GEMM_SWZ": "0"},
}
GEMM_SHAPES = [(1, 1, 1), (1, 130, 17), (131, 1, 16), (64, 64, 0), (129, 257, 33), (67, 35, 5),
               (200, 137, 50)]


def set_env(monkeypatch, env):
    for k in ("TG_GEMM_TILE", "TG_GEMM_IMPL", "TG_GEMM_SWZ"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_dgemm_exact(L, monkeypatch, kernel, ta, tb):
    """Every forced kernel, transposition, edge shape (one element, one row, one
    column, K = 0, K below a slab, ragged tiles) and layout; K = 0 gives beta C0."""
    set_env(monkeypatch, KERNELS[kernel])
    rng = np.random.default_rng(1)
    seen, i = set(), 0
    for M, N, K in GEMM_SHAPES:
        for lays in LAYS + LAYS_MIXED:
            for j in range(3):
                alpha, beta = AB[(i + 2 * j) % 6]
                gemm_case(L, GEMM, ta, tb, M, N, K, alpha, beta, lays, rng, True, seen=seen)
            i += 1
    if "own8" in kernel:  # all four VA / VB instances of the 8-wave kernel ran
        assert seen == {(False, False), (False, True), (True, False), (True, True)}


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_dgemm_bounded(L, monkeypatch, kernel, ta, tb):
    set_env(monkeypatch, KERNELS[kernel])
    rng = np.random.default_rng(2)
    worst = 0.0
    for M, N, K in GEMM_SHAPES:
        for lays in (LAYS[2], LAYS[3]):
            for alpha, beta in ((0.7, 0.0), (-1.3, 0.6)):
                worst = max(worst, gemm_case(L, GEMM, ta, tb, M, N, K, alpha, beta, lays, rng,
                                             False, entry="tg_dgemm"))
    print(f"dgemm {kernel} ta={ta} tb={tb}: worst err/bound = {worst:.3g}")


@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("swz", ["1", "0"])
def test_dgemm8_tile_map(L, monkeypatch, swz, ta, tb):
    """10 x 3 tiles of 128: the swizzled map's last row group has 2 rows, and
    nb = 30 is no multiple of the 8 ranges the tiles are dealt into."""
    M, N, K = 1153, 257, 20
    assert (-(-M // 128), -(-N // 128)) == (10, 3)
    set_env(monkeypatch, {"TG_GEMM_TILE": "128", "TG_GEMM_IMPL": "own8", "TG_GEMM_SWZ": swz})
    rng = np.random.default_rng(3)
    for lays, (alpha, beta) in ((LAYS[3], AB[0]), (LAYS[2], AB[2])):
        gemm_case(L, GEMM, ta, tb, M, N, K, alpha, beta, lays, rng, True)


# ---- dgemm_upper_a -----------------------------------------------------------
UPA_SHAPES = [(1, 1, 1), (65, 30, 65), (130, 70, 130), (130, 200, 150)]


@pytest.mark.parametrize("tile", [64, 128])
def test_dgemm_upper_a(L, monkeypatch, tile):
    """A upper triangular with NaN strictly below its tile-sized diagonal blocks
    (module docstring): the skipped part of the triangle must not reach C."""
    set_env(monkeypatch, {"TG_GEMM_TILE": str(tile)})
    rng = np.random.default_rng(4)
    worst, i = 0.0, 0
    for M, N, K in UPA_SHAPES:
        for lays in LAYS + LAYS_MIXED:
            for j in range(3):
                alpha, beta = AB[(i + 2 * j) % 6]
                gemm_case(L, UPPER_A, 0, 0, M, N, K, alpha, beta, lays, rng, True, tile=tile)
            i += 1
        for lays in (LAYS[2], LAYS[3]):
            for alpha, beta in ((0.7, 0.0), (-1.3, 0.6)):
                worst = max(worst, gemm_case(L, UPPER_A, 0, 0, M, N, K, alpha, beta, lays, rng,
                                             False, tile=tile))
    print(f"dgemm_upper_a tile {tile}: worst err/bound = {worst:.3g}")


# ---- dgemm_splitk ------------------------------------------------------------
# the fall-back K < 32 splits: (32, 40, 100) from splits = 7, (32, 64, 95) from 3;
# K no multiple of the chunk: 999, 95, 100; fewer chunks than splits: K = 225 with
# splits = 7 (chunk 48 -> 5 chunks; the scratch slices 5 and 6 keep their NaN)
SPLITK_SHAPES = [(32, 40, 100), (32, 70, 1000), (33, 65, 999), (32, 64, 95), (32, 64, 225)]


@pytest.mark.parametrize("splits", [1, 2, 3, 7])
@pytest.mark.parametrize("ta,tb", TRANS)
def test_dgemm_splitk(L, monkeypatch, ta, tb, splits):
    """The scratch is NaN beforehand: every slice that is summed was written."""
    set_env(monkeypatch, {})
    rng = np.random.default_rng(5)
    worst, i = 0.0, 0
    for M, N, K in SPLITK_SHAPES:
        for lays in LAYS:
            alpha, beta = AB[i % 6]
            gemm_case(L, SPLITK, ta, tb, M, N, K, alpha, beta, lays, rng, True, splits=splits)
            i += 1
        for alpha, beta in ((0.7, 0.0), (-1.3, 0.6)):
            worst = max(worst, gemm_case(L, SPLITK, ta, tb, M, N, K, alpha, beta, LAYS[2], rng,
                                         False, splits=splits))
    print(f"dgemm_splitk splits={splits} ta={ta} tb={tb}: worst err/bound = {worst:.3g}")


# ---- sum_partials ------------------------------------------------------------
@pytest.mark.parametrize("nz", [1, 5])
@pytest.mark.parametrize("M,N", [(1, 1), (37, 32), (300, 33)])
def test_sum_partials(L, nz, M, N):
    """C = alpha sum_z P_z + beta C with ldc > N; P (nz slices, ld N) at the
    start of an allocation and one element into it."""
    rng = np.random.default_rng(6)
    i = 0
    for lead in (0, 1):
        for lc in ("A", "B", "V"):
            for alpha, beta in AB[i % 2::2]:
                Ph, C0 = ints(rng, (nz * M, N)), ints(rng, (M, N), 8)
                P = Dev(Ph, "C")
                P.lead, (P.p, P.buf) = lead, padded(Ph, N, lead)
                P.before = P.buf.clone()
                C = Dev(c_init(C0, beta), lc)
                assert C.ld > N
                probe(L, SUM_PARTIALS, 0, 0, M, N, 0, alpha, P, None, beta, C, splits=nz)
                ref = R.axpby(alpha, Ph.reshape(nz, M, N).astype(np.int64).sum(0), beta, C0)
                got = C.get()
                assert C.intact() and P.unchanged()
                assert np.array_equal(got, ref), R.first_mismatch(got, ref)
            i += 1
    # standard-normal partials: an nz-term sum
    Ph, C0 = rng.standard_normal((nz * M, N)), rng.standard_normal((M, N))
    P, C = Dev(Ph, "C"), Dev(C0, "B")
    probe(L, SUM_PARTIALS, 0, 0, M, N, 0, 0.7, P, None, -1.3, C, splits=nz)
    P3 = Ph.reshape(nz, M, N)
    ref = 0.7 * P3.sum(0) + -1.3 * C0
    bound = 2.0 * (nz + 3) * R.U * (0.7 * np.abs(P3).sum(0) + 1.3 * np.abs(C0))
    ratio = R.worst_ratio(C.get(), ref, bound)
    print(f"sum_partials nz={nz} {M}x{N}: worst err/bound = {ratio:.3g}")
    assert ratio <= 1.0 and C.intact()


# ---- SYRK --------------------------------------------------------------------
SYRK_LAYS = [("C", "C"), ("B", "B"), ("V", "V"), ("V", "B")]


def sym(C0):
    return np.tril(C0) + np.tril(C0, -1).T


def syrk_case(L, op, n, K, alpha, beta, lays, rng, exact):
    """One SYRK call.  TN / TN_LOWER: X is K x n; NT: X is n x K; TN_UPPER: X is
    n x n upper triangular with exact zeros below (K = n)."""
    gen = ints if exact else (lambda r, s, lim=None: r.standard_normal(s))
    Xh = gen(rng, (n, K) if op == SYRK_NT else (K, n))
    if op == SYRK_TN_UPPER:
        Xh = np.triu(Xh)
    C0 = sym(gen(rng, (n, n), 8))
    ta, tb = (0, 1) if op == SYRK_NT else (1, 0)
    if exact:
        ref, bound = R.gemm_exact(ta, tb, alpha, Xh, Xh, beta, C0), None
    else:
        ref, bound = R.gemm_bound(ta, tb, alpha, Xh, Xh, beta, C0)
    init = c_init(C0, beta)
    if op == SYRK_TN_LOWER:  # outside the lower and diagonal tiles nothing is written
        mask = R.syrk_lower_mask(n)
        init, ref = np.where(mask, init, SENTINEL), np.where(mask, ref, SENTINEL)
        if bound is not None:
            bound = np.where(mask, bound, 0.0)
    X = Dev(Xh, lays[0])
    outs = []
    for _ in range(1 if exact else 2):
        C = Dev(init, lays[1])
        probe(L, op, 0, 0, 0, n, K, alpha, X, None, beta, C)
        got = C.get()
        what = (op, n, K, alpha, beta, lays)
        assert C.intact(), f"wrote outside the logical C: {what}"
        assert X.unchanged(), f"X changed: {what}"
        assert np.all(np.isfinite(got)), f"non-finite result: {what}"
        if op != SYRK_TN_LOWER:
            assert np.array_equal(got, got.T), f"C is not symmetric bit for bit: {what}"
        outs.append(got)
    if exact:
        assert np.array_equal(outs[0], ref), f"{what}: {R.first_mismatch(outs[0], ref)}"
        return 0.0
    assert np.array_equal(outs[0], outs[1]), f"two calls differ: {what}"
    ratio = R.worst_ratio(outs[0], ref, bound)
    assert ratio <= 1.0, f"err/bound {ratio:.3f}: {what}"
    return ratio


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 200])
@pytest.mark.parametrize("op", [SYRK_TN, SYRK_NT, SYRK_TN_LOWER],
                         ids=["dsyrk_tn", "dsyrk_nt", "dsyrk_tn_lower"])
def test_syrk_small(L, monkeypatch, op, n):
    """The 64-tile SYRKs: mirrored forms equal the reference and their own
    transpose bit for bit; dsyrk_tn_lower writes its lower and diagonal tiles
    and leaves the sentinel everywhere else of the logical C."""
    set_env(monkeypatch, {})
    rng = np.random.default_rng(7)
    worst, i = 0.0, 0
    for K in (1, 17, 64):
        for lays in SYRK_LAYS:
            for j in range(3):
                alpha, beta = AB[(i + 2 * j) % 6]
                syrk_case(L, op, n, K, alpha, beta, lays, rng, True)
            i += 1
        for alpha, beta in ((0.7, 0.0), (-1.3, 0.6)):
            worst = max(worst, syrk_case(L, op, n, K, alpha, beta, SYRK_LAYS[3], rng, False))
    print(f"syrk op {op} n={n}: worst err/bound = {worst:.3g}")


@pytest.mark.parametrize("n", [1, 127, 129, 300])
@pytest.mark.parametrize("impl", ["own8", "own"])
def test_syrk_tn_upper(L, monkeypatch, impl, n):
    """X upper triangular, K = n: own8 runs the 8-wave SYRK that sums only
    k < tn + 128 of each tile, own falls back to dsyrk_tn; both give X^T X."""
    set_env(monkeypatch, {"TG_GEMM_IMPL": impl})
    rng = np.random.default_rng(8)
    worst = 0.0
    for i, lays in enumerate(SYRK_LAYS):
        for j in range(3):
            alpha, beta = AB[(i + 2 * j) % 6]
            syrk_case(L, SYRK_TN_UPPER, n, n, alpha, beta, lays, rng, True)
        worst = max(worst, syrk_case(L, SYRK_TN_UPPER, n, n, 0.7, (0.0, -1.3)[i % 2], lays, rng,
                                     False))
    print(f"dsyrk_tn_upper {impl} n={n}: worst err/bound = {worst:.3g}")


BIG_N, BIG_K = 5760, 24  # 45 tiles of 128 per side: 1035 >= 1024 lower tiles


@pytest.fixture(scope="module")
def big_syrk():
    """X (K x n integers) and X^T X in int64, computed once for the three cases."""
    rng = np.random.default_rng(9)
    Xh = ints(rng, (BIG_K, BIG_N))
    Xi = Xh.astype(np.int64)
    return Xh, (Xi.T @ Xi).astype(np.float64)


@pytest.mark.parametrize("impl,ldx", [("own8", BIG_N), ("own8", BIG_N + 1), ("own", BIG_N)],
                         ids=["own8-vec", "own8-odd-ldx", "own-4wave"])
def test_syrk_128_tiles(L, monkeypatch, big_syrk, impl, ldx):
    """The 128-tile SYRKs dsyrk_tn takes from 1024 lower tiles (n >= 5633):
    the 8-wave kernel without the K-cut, with 16-byte and with 8-byte loads,
    and the 4-wave 128 x 128 kernel.  Exact, NaN-prefilled C, padded ldc."""
    n128 = -(-BIG_N // 128)
    assert n128 * (n128 + 1) // 2 >= 1024 > (n128 - 1) * n128 // 2
    set_env(monkeypatch, {"TG_GEMM_IMPL": impl})
    Xh, S = big_syrk
    X = Dev(Xh, "C")
    X.ld, (X.p, X.buf) = ldx, padded(Xh, ldx, 0)
    X.before = X.buf.clone()
    assert (X.p.value % 16 == 0 and ldx % 2 == 0) == (ldx == BIG_N)
    ldc = BIG_N + 8
    p, buf = padded(np.full((BIG_N, BIG_N), np.nan), ldc, 0)
    L.call("tg_gemm64_probe", L.stream(), SYRK_TN, 0, 0, 0, BIG_N, BIG_K, 0.5, X.p, ldx, None, 0,
           0.0, p, ldc, 0, None, 0)
    flat = buf.cpu().numpy()
    got = flat[:BIG_N * ldc].reshape(BIG_N, ldc)
    assert np.all(got[:, BIG_N:] == SENTINEL) and np.all(flat[BIG_N * ldc:] == SENTINEL)
    got = got[:, :BIG_N]
    assert X.unchanged()
    assert np.array_equal(got, 0.5 * S), R.first_mismatch(got, 0.5 * S)
    assert np.array_equal(got, got.T)


# ---- dgemm_chunked -----------------------------------------------------------
def chunked_case(L, ta, tb, mkspec, shapes, lays, alpha, beta, rng, exact, tri=0, tile=None,
                 stack=None):
    """One tg_gemm64_chunked call checked on the whole flat image of C (result,
    padding and everything between the chunks' blocks).  mkspec(lda, ldb, ldc)
    gives the 12 spec values; stack = (b, nc): operand A (tri 1) or B (tri 2) is
    a stack of upper-triangular b x b blocks poisoned below their tile-sized
    diagonal blocks.  Returns the worst err / bound."""
    gen = ints if exact else (lambda r, s, lim=None: r.standard_normal(s))
    Ah, Bh, C0 = gen(rng, shapes[0]), gen(rng, shapes[1]), gen(rng, shapes[2], 8)
    if tri:
        b, nc = stack
        blocks = (Ah if tri == 1 else Bh).reshape(nc, b, b)
        for z in range(nc):
            blocks[z] = R.tri_nan(blocks[z], tile)
    A, B = Dev(Ah, lays[0]), Dev(Bh, lays[1])
    spec = mkspec(A.ld, B.ld, R.place(shapes[2][1], lays[2])[1])
    outs = []
    for _ in range(1 if exact else 2):
        C = Dev(c_init(C0, beta), lays[2])
        want = C.flat()
        # the reference first: it asserts that every chunk stays inside its buffers
        bound = R.chunked_apply(ta, tb, spec, alpha, A.flat(), A.lead, A.ld, B.flat(), B.lead, B.ld,
                                beta, want, C.lead, C.ld, exact=exact, tri=tri)
        L.call("tg_gemm64_chunked", L.stream(), ta, tb, (ctypes.c_int64 * 12)(*spec), tri, alpha,
               A.p, A.ld, B.p, B.ld, beta, C.p, C.ld)
        got = C.flat()
        what = (ta, tb, spec, tri, alpha, beta, lays)
        assert C.intact(), f"wrote outside the logical C: {what}"
        assert A.unchanged() and B.unchanged(), f"an input changed: {what}"
        outs.append(got)
    written = bound > 0 if not exact else None
    if exact:
        assert R.first_mismatch(got, want) is None, f"{what}: {R.first_mismatch(got, want)}"
        assert np.all(np.isfinite(C.get())), f"non-finite result: {what}"
        return 0.0
    assert np.array_equal(outs[0], outs[1], equal_nan=True), f"two calls differ: {what}"
    assert np.count_nonzero(written) == sum(M * N for _, _, _, M, N, _ in R.chunks(spec))
    assert R.first_mismatch(got[~written], want[~written]) is None, f"stray write: {what}"
    ratio = R.worst_ratio(got[written], want[written], bound[written])
    assert ratio <= 1.0, f"err/bound {ratio:.3f}: {what}"
    return ratio


def chunked_all(L, name, ta, tb, mkspec, shapes, rng, **kw):
    for i, lays in enumerate(LAYS):
        chunked_case(L, ta, tb, mkspec, shapes, lays, *AB[i % 6], rng, True, **kw)
        chunked_case(L, ta, tb, mkspec, shapes, lays, *AB[(i + 3) % 6], rng, True, **kw)
    worst = max(chunked_case(L, ta, tb, mkspec, shapes, LAYS[2], 0.7, beta, rng, False, **kw)
                for beta in (0.0, -1.3))
    print(f"dgemm_chunked {name}: worst err/bound = {worst:.3g}")


SB_B, SB_C = 32, 256  # band.hip's panel width and chunk length


def test_chunked_band_level0(L):
    """X = A22 blockdiag(YT): NN, the 32-wide narrow tile, K = the chunk length;
    the last chunk has 88 rows."""
    m = 600
    chunked_all(L, "band level 0 (NN, narrow)", 0, 0,
                lambda lda, ldb, ldc: [SB_C, 3, m, 1, 0, ldb, 0, 0, SB_B, m, SB_B, -1],
                [(m, m), (m, SB_B), (m, 3 * SB_B)], np.random.default_rng(10))


def test_chunked_tn_partials_and_sum(L):
    """X = sum_z A22[block z, :]^T YT[32 z : 32 z + 32, :]: 32-row blocks of A at
    a stride of 96 rows, TN, five partial products, then sum_partials."""
    m, nz = 200, 5
    rng = np.random.default_rng(11)
    chunked_all(L, "TN partials", 1, 0,
                lambda lda, ldb, ldc: [SB_B, nz, nz * SB_B, 3 * lda, 0, ldb, 0, 0, m * ldc, m, SB_B,
                                       SB_B],
                [(4 * 96 + SB_B, m), (nz * SB_B, SB_B), (nz * m, SB_B)], rng)
    # the product's pipeline: contiguous partials (ld 32), summed into a padded X
    Ah, Bh = ints(rng, (4 * 96 + SB_B, m)), ints(rng, (nz * SB_B, SB_B))
    A, B = Dev(Ah, "B"), Dev(Bh, "C")
    P = Dev(np.full((nz * m, SB_B), np.nan), "C")
    X = Dev(np.full((m, SB_B), np.nan), "V")
    spec = [SB_B, nz, nz * SB_B, 3 * A.ld, 0, SB_B, 0, 0, m * SB_B, m, SB_B, SB_B]
    L.call("tg_gemm64_chunked", L.stream(), 1, 0, (ctypes.c_int64 * 12)(*spec), 0, 1.0, A.p, A.ld,
           B.p, B.ld, 0.0, P.p, P.ld)
    probe(L, SUM_PARTIALS, 0, 0, m, SB_B, 0, 1.0, P, None, 0.0, X, splits=nz)
    ref = sum(R.exact_product(Ah[96 * z:96 * z + SB_B].T, Bh[SB_B * z:SB_B * (z + 1)])
              for z in range(nz)).astype(np.float64)
    assert np.array_equal(X.get(), ref) and X.intact() and P.intact()


def test_chunked_tn_k(L):
    """X = Gr^T blockdiag(YT): TN with K = the chunk length (256, then 44)."""
    m = 200
    chunked_all(L, "TN, K = chunk", 1, 0,
                lambda lda, ldb, ldc: [SB_C, 2, 300, lda, 0, ldb, 0, 0, SB_B, m, SB_B, -1],
                [(300, m), (300, SB_B), (m, 2 * SB_B)], np.random.default_rng(12))


@pytest.mark.parametrize("m", [200, 40])
def test_chunked_nt_m(L, m):
    """U = Y W^T: NT with M = the chunk length; m = 200 runs 64-wide tiles over
    several columns, m = 40 a single column of them."""
    chunked_all(L, f"NT, M = chunk, m={m}", 0, 1,
                lambda lda, ldb, ldc: [SB_C, 2, 300, lda, 0, 0, SB_B, ldc, 0, -1, m, SB_B],
                [(300, SB_B), (m, 2 * SB_B), (300, m)], np.random.default_rng(13))


def test_chunked_nt_m_128_tiles(L):
    """U = Y W^T with chunks of 130 rows and m = 130: 2 * 2 * 64 = 256 tiles of
    128 select the 128-tile instance (the product: m = 2048 with 8 chunks)."""
    c, nc, m = 130, 64, 130
    rows = c * (nc - 1) + 77
    rng = np.random.default_rng(16)
    mk = lambda lda, ldb, ldc: [c, nc, rows, lda, 0, 0, SB_B, ldc, 0, -1, m, SB_B]  # noqa: E731
    shapes = [(rows, SB_B), (m, nc * SB_B), (rows, m)]
    for i, lays in enumerate((LAYS[2], LAYS[3])):
        chunked_case(L, 0, 1, mk, shapes, lays, *AB[2 + i], rng, True)
    worst = chunked_case(L, 0, 1, mk, shapes, LAYS[2], 0.7, -1.3, rng, False)
    print(f"dgemm_chunked NT, M = chunk, 128 tiles: worst err/bound = {worst:.3g}")


@pytest.mark.parametrize("ta,tb", TRANS)
def test_chunked_stack_128_tiles(L, ta, tb):
    """64 independent 130 x 130 x 20 products (c = 1: chunk z is problem z), the
    128-tile instance of every transposition."""
    M = N = 130
    K, nc = 20, 64
    ra, rb = (K if ta else M), (N if tb else K)
    rng = np.random.default_rng(17)
    mk = lambda lda, ldb, ldc: [1, nc, nc, ra * lda, 0, rb * ldb, 0, M * ldc, 0, M, N, K]  # noqa: E731
    shapes = [(nc * ra, M if ta else K), (nc * rb, K if tb else N), (nc * M, N)]
    for i, lays in enumerate((LAYS[2], LAYS[3])):
        chunked_case(L, ta, tb, mk, shapes, lays, *AB[i], rng, True)
    worst = chunked_case(L, ta, tb, mk, shapes, LAYS[2], 0.7, -1.3, rng, False)
    print(f"dgemm_chunked stack ta={ta} tb={tb}, 128 tiles: worst err/bound = {worst:.3g}")


# b = 64, nc = 3: the 64-tile (one tile: no skipped triangle); b = 130, nc = 3: 3 x 3
# tiles of 64 with one; b = 130, nc = 64: 2 * 2 * 64 = 256 tiles of 128, the 128-tile
@pytest.mark.parametrize("b,nc,tile", [(64, 3, 64), (130, 3, 64), (130, 64, 128)])
@pytest.mark.parametrize("tri", [1, 2])
def test_chunked_tri(L, tri, b, nc, tile):
    """Stacks of independent b x b problems with A (tri 1) or B (tri 2) upper
    triangular, NaN strictly below the tile-sized diagonal blocks."""
    assert ((-(-b // 128)) ** 2 * nc >= 256 and b > 64) == (tile == 128)
    rng = np.random.default_rng(14)
    mk = lambda lda, ldb, ldc: [b, nc, b * nc, lda, 0, ldb, 0, ldc, 0, b, b, b]  # noqa: E731
    shapes = [(b * nc, b)] * 3
    kw = dict(tri=tri, tile=tile, stack=(b, nc))
    lays = LAYS if nc < 64 else [LAYS[2], LAYS[3]]
    for i, ls in enumerate(lays):
        chunked_case(L, 0, 0, mk, shapes, ls, *AB[(i + tri) % 6], rng, True, **kw)
        chunked_case(L, 0, 0, mk, shapes, ls, *AB[(i + tri + 3) % 6], rng, True, **kw)
    worst = max(chunked_case(L, 0, 0, mk, shapes, LAYS[2], 0.7, beta, rng, False, **kw)
                for beta in (0.0, -1.3))
    print(f"dgemm_chunked tri={tri} b={b} nc={nc}: worst err/bound = {worst:.3g}")


@pytest.mark.parametrize("lay", ["B", "V"])
@pytest.mark.parametrize("b", [64, 128])
def test_chunked_trinv_offdiag_specs(L, b, lay):
    """The two launches of one level of the triangular inverse at n = 512: on a
    real upper-triangular U, with the b x b diagonal blocks of Y = U^-1 in
    place, T_p = Y11 U12 (tri 1) and Y12 = -T_p Y22 (tri 2) for every pair p of
    adjacent blocks; T and the Y12 blocks are NaN beforehand."""
    n = 512
    nfull = n // (2 * b)
    rng = np.random.default_rng(15)
    Uh = np.triu(rng.standard_normal((n, n))) / np.sqrt(n) + 2.0 * np.eye(n)
    Yh = np.zeros((n, n))
    for s in range(0, n, b):
        Yh[s:s + b, s:s + b] = np.triu(np.linalg.inv(Uh[s:s + b, s:s + b]))
    for q in range(nfull):
        s = 2 * b * q
        Yh[s:s + b, s + b:s + 2 * b] = np.nan
    U, Y = Dev(Uh, lay), Dev(Yh, lay)
    T = Dev(np.full((nfull * b, b), np.nan), "C")
    dy, du = Y.ld + 1, U.ld + 1
    c1 = [2 * b, nfull, 2 * b * nfull, dy, 0, du, 0, 0, b * T.ld, b, b, b]
    c2 = [2 * b, nfull, 2 * b * nfull, 0, b * T.ld, dy, 0, dy, 0, b, b, b]
    # stage 1 against its own reference and bound
    wantT = T.flat()
    bound1 = R.chunked_apply(0, 0, c1, 1.0, Y.flat(), Y.lead, Y.ld, U.flat(), U.lead + b, U.ld,
                             0.0, wantT, T.lead, T.ld, exact=False, tri=1)
    L.call("tg_gemm64_chunked", L.stream(), 0, 0, (ctypes.c_int64 * 12)(*c1), 1, 1.0, Y.p, Y.ld,
           U.at(b), U.ld, 0.0, T.p, T.ld)
    gotT = T.flat()
    assert T.intact() and Y.unchanged() and U.unchanged()
    T.before = T.buf.clone()
    assert np.count_nonzero(bound1 > 0) == nfull * b * b   # every entry of every T_p is judged
    r1 = R.worst_ratio(gotT[bound1 > 0], wantT[bound1 > 0], bound1[bound1 > 0])
    # stage 2 from the device's T
    wantY = Y.flat()
    bound2 = R.chunked_apply(0, 0, c2, -1.0, gotT, T.lead, T.ld, Y.flat(), Y.lead + b * Y.ld + b,
                             Y.ld, 0.0, wantY, Y.lead + b, Y.ld, exact=False, tri=2)
    L.call("tg_gemm64_chunked", L.stream(), 0, 0, (ctypes.c_int64 * 12)(*c2), 2, -1.0, T.p, T.ld,
           Y.at(b * Y.ld + b), Y.ld, 0.0, Y.at(b), Y.ld)
    gotY = Y.flat()
    w = bound2 > 0
    assert np.count_nonzero(w) == nfull * b * b
    assert Y.intact() and T.unchanged() and U.unchanged()
    assert R.first_mismatch(gotY[~w], wantY[~w]) is None, "wrote outside the Y12 blocks"
    r2 = R.worst_ratio(gotY[w], wantY[w], bound2[w])
    # both together against Y12 = -(Y11 U12) Y22 in numpy: the error of T_p
    # (<= bound1) passes through |Y22|, on top of the second product's own bound
    Yg, r3 = Y.get(), 0.0
    for q in range(nfull):
        s = 2 * b * q
        Y11, Y22 = Yh[s:s + b, s:s + b], Yh[s + b:s + 2 * b, s + b:s + 2 * b]
        U12 = Uh[s:s + b, s + b:s + 2 * b]
        Tp = Y11 @ U12
        e1 = 2.0 * (b + 3) * R.U * (np.abs(Y11) @ np.abs(U12))
        bound = 2.0 * (b + 3) * R.U * ((np.abs(Tp) + e1) @ np.abs(Y22)) + e1 @ np.abs(Y22)
        r3 = max(r3, R.worst_ratio(Yg[s:s + b, s + b:s + 2 * b], -Tp @ Y22, bound))
    print(f"trinv_offdiag specs b={b} {lay}: worst err/bound = {r1:.3g} (Y11 U12), "
          f"{r2:.3g} (T Y22), {r3:.3g} (both)")
    assert r1 <= 1.0 and r2 <= 1.0 and r3 <= 1.0
