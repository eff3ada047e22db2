"""Host references and checks for the FP64 GEMM family tests
(test_gpu_gemm64_family.py; self-tested without a GPU in test_gemm64_refs.py).

Everything here works on the *flat* host image of a padded operand, laid out
as abi_helpers.padded() lays it out on the device: `lead` sentinel elements, a
rows x width matrix with row stride ld, the columns width .. ld-1 and TAIL
further elements holding the sentinel.  A reference is applied to a copy of
the output's flat image, so comparing the whole image afterwards checks the
result and "nothing outside the logical matrix was written" in one go.

Two kinds of reference:
  exact    small-integer operands, alpha and beta powers of two: every product
           and every partial sum is an exact double in any summation order, so
           the kernel must reproduce numpy's int64 result bit for bit;
  bounded  standard-normal operands against numpy's FP64 product with the
           first-order any-order bound of a K-term FP64 dot product plus the
           alpha / beta roundings, |C - C_ref| <= 2 (K + 3) 2^-53 (|alpha| |op A|
           |op B| + |beta| |C0|) per element (the factor 2: the numpy reference
           is an FP64 sum in some order too).
"""
import numpy as np

from abi_helpers import LAYOUTS, SENTINEL, TAIL

U = 2.0 ** -53


def place(width, layout):
    """(lead, ld) of a matrix of `width` columns in `layout`: abi_helpers.LAYOUTS
    plus V, the base at the start of the allocation and an even ld > width, so
    the 16-byte load path is taken (vec_ok) and, with an odd width, the last
    pair of a row lies half outside the logical matrix."""
    if layout == "V":
        return 0, width + (1 if width % 2 else 2)
    lead, pad = LAYOUTS[layout]
    return lead, width + pad


def flat_image(a, ld, lead, sentinel=SENTINEL):
    """The host image abi_helpers.padded(a, ld, lead) uploads."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    rows, width = a.shape
    flat = np.full(lead + rows * ld + TAIL, sentinel, dtype=np.float64)
    flat[lead:lead + rows * ld].reshape(rows, ld)[:, :width] = a
    return flat


def view(flat, off, rows, cols, ld):
    """Writable rows x cols window of `flat` at element offset `off`, stride ld."""
    if rows == 0 or cols == 0:
        return np.zeros((rows, cols))
    assert off >= 0 and off + (rows - 1) * ld + cols <= flat.size, "window leaves the buffer"
    return np.lib.stride_tricks.as_strided(flat[off:], (rows, cols),
                                           (ld * flat.itemsize, flat.itemsize))


def op(X, trans):
    return X.T if trans else X


def exact_product(A, B):
    """A B in int64 for integer-valued operands (exact)."""
    Ai, Bi = np.rint(A).astype(np.int64), np.rint(B).astype(np.int64)
    assert np.array_equal(Ai, A) and np.array_equal(Bi, B), "exact reference needs integers"
    return Ai @ Bi


def axpby(alpha, P, beta, C0):
    """alpha P + beta C0, C0 not read when beta == 0 (the kernels' contract)."""
    P = np.asarray(P, dtype=np.float64)
    return alpha * P if beta == 0.0 else alpha * P + beta * C0


def assert_exact_range(alpha, A, B, beta, C0):
    """The magnitudes stay below 2^53: every intermediate is an exact double."""
    top = abs(alpha) * (np.abs(A) @ np.abs(B)) if A.shape[1] else np.zeros((A.shape[0], B.shape[1]))
    if beta != 0.0:
        top = top + abs(beta) * np.abs(C0)
    assert top.size == 0 or np.max(top) < 2.0 ** 53


def gemm_exact(ta, tb, alpha, A, B, beta, C0):
    oa, ob = op(A, ta), op(B, tb)
    assert_exact_range(alpha, oa, ob, beta, C0)
    return axpby(alpha, exact_product(oa, ob), beta, C0)


def gemm_bound(ta, tb, alpha, A, B, beta, C0):
    """(FP64 reference, per-element bound) of alpha op(A) op(B) + beta C0."""
    oa, ob = op(A, ta), op(B, tb)
    K = oa.shape[1]
    ref = axpby(alpha, oa @ ob, beta, C0)
    mag = abs(alpha) * (np.abs(oa) @ np.abs(ob))
    if beta != 0.0:
        mag = mag + abs(beta) * np.abs(C0)
    return ref, 2.0 * (K + 3) * U * mag


def worst_ratio(C, ref, bound):
    """max |C - ref| / bound (0 / 0 counts as 0; anything non-finite as inf)."""
    if C.size == 0:
        return 0.0
    if not np.all(np.isfinite(C)):
        return np.inf
    err = np.abs(C - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r))


def chunks(spec):
    """[(z, kb, h, M, N, K)] of a ChunkSpec (c, nc, m, a_kb, a_z, b_kb, b_z, c_kb, c_z, M, N, K)."""
    c, nc, m = spec[0], spec[1], spec[2]
    out = []
    for z in range(nc):
        kb = z * c
        ke = m if z == nc - 1 else kb + c
        h = ke - kb
        M, N, K = (h if v < 0 else v for v in spec[9:12])
        out.append((z, kb, h, M, N, K))
    return out


def chunked_apply(ta, tb, spec, alpha, Af, a0, lda, Bf, b0, ldb, beta, Cf, c0, ldc, exact=True,
                  tri=0):
    """Apply the chunked GEMM to the flat image Cf in place (A, B, C start at
    the element offsets a0, b0, c0 of their flat images).  With exact=False it
    returns the flat image of the error bounds as well (0 where nothing is
    written).  tri = 1 / 2: A_z / B_z is upper triangular whatever its lower
    triangle holds (tri_nan poisons it); the reference multiplies the triangle."""
    a_kb, a_z, b_kb, b_z, c_kb, c_z = spec[3:9]
    Bd = np.zeros_like(Cf)
    for z, kb, h, M, N, K in chunks(spec):
        A = view(Af, a0 + kb * a_kb + z * a_z, *((K, M) if ta else (M, K)), lda)
        B = view(Bf, b0 + kb * b_kb + z * b_z, *((N, K) if tb else (K, N)), ldb)
        C = view(Cf, c0 + kb * c_kb + z * c_z, M, N, ldc)
        if tri == 1:
            A = np.triu(np.nan_to_num(A, nan=0.0))
        if tri == 2:
            B = np.triu(np.nan_to_num(B, nan=0.0))
        if exact:
            C[...] = gemm_exact(ta, tb, alpha, A, B, beta, C.copy())
        else:
            ref, bound = gemm_bound(ta, tb, alpha, A, B, beta, C.copy())
            C[...] = ref
            view(Bd, c0 + kb * c_kb + z * c_z, M, N, ldc)[...] = bound
    return Bd


def chunked_loops(ta, tb, spec, alpha, Af, a0, lda, Bf, b0, ldb, beta, Cf, c0, ldc):
    """The same as chunked_apply(exact=True), as plain loops over scalars
    (self-test of the reference builder; tiny sizes only)."""
    a_kb, a_z, b_kb, b_z, c_kb, c_z = spec[3:9]
    for z, kb, h, M, N, K in chunks(spec):
        ao, bo, co = a0 + kb * a_kb + z * a_z, b0 + kb * b_kb + z * b_z, c0 + kb * c_kb + z * c_z
        for i in range(M):
            for j in range(N):
                s = 0.0
                for k in range(K):
                    a = Af[ao + k * lda + i] if ta else Af[ao + i * lda + k]
                    b = Bf[bo + j * ldb + k] if tb else Bf[bo + k * ldb + j]
                    s += a * b
                s *= alpha
                if beta != 0.0:
                    s += beta * Cf[co + i * ldc + j]
                Cf[co + i * ldc + j] = s


def tri_nan(X, tile, fill=np.nan):
    """An upper-triangular operand whose unread zeros are poisoned: zeros stay
    inside the tile x tile diagonal blocks (a tile row / column sums from / up
    to its own diagonal block, so those zeros are multiplied), `fill` strictly
    below the diagonal blocks, where a kernel that honours the K-cut never
    reads."""
    X = np.triu(X).astype(np.float64)
    r, c = np.indices(X.shape)
    X[(r // tile) > (c // tile)] = fill
    return X


def syrk_lower_mask(n, tile=64):
    """True where dsyrk_tn_lower writes: the lower and diagonal tile x tile tiles."""
    r, c = np.indices((n, n))
    return (r // tile) >= (c // tile)


def first_mismatch(got, want):
    """None when the two flat images agree (NaN == NaN), else a description."""
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad)[0])
    return f"{int(bad.sum())} elements differ, first at flat index {i}: {got[i]!r} != {want[i]!r}"


# ---- a numpy emulation of a tiled kernel with injectable faults --------------
def emulate(flatC, lead, ldc, n_rows, n_cols, alpha, oa, ob, beta, fault=None, syrk=False, kc=16,
            tile=64):
    """What a tiled kernel would leave in the flat image of C, for the
    self-test of the checks: fault = None | "drop_slab" (the last k-slab of kc
    is not summed) | "no_mirror" (syrk: one off-diagonal tile is not mirrored) |
    "pad_write" (the first row is written one column too far)."""
    K = oa.shape[1]
    kend = K - (K % kc or kc) if fault == "drop_slab" else K
    C = view(flatC, lead, n_rows, n_cols, ldc)
    C0 = C.copy()
    new = axpby(alpha, oa[:, :kend] @ ob[:kend, :], beta, C0)
    if syrk:
        low = np.tril(new)
        new = low + np.tril(new, -1).T
        if fault == "no_mirror":
            new[:tile, tile:2 * tile] = C0[:tile, tile:2 * tile]
    C[...] = new
    if fault == "pad_write":
        flatC[lead + n_cols] = new[0, 0]
    return flatC
