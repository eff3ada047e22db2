"""CPU: every C-ABI entry point rejects a bad argument before any device work.

include/truncgptq.h: "<0 invalid argument (-(1-based argument index))" and
tg_last_error() names it.  Each case below starts from a call whose arguments
are all acceptable (placeholder non-null pointers: nothing is dereferenced on
the host) and replaces exactly one of them: a null pointer, a size out of
range, or a leading dimension one short of the width.  The call must return
-(index of that argument) and the message must say "argument <index>".  No
device exists here, so a case that slipped through validation would show as a
positive hipError_t instead.
"""
import ctypes

import pytest

P = 16           # placeholder non-null pointer
BIG = 1 << 40    # workspace byte count no size check can object to


@pytest.fixture(scope="module")
def L():
    import gptq_svd_amd._lib as L
    return L


TRIES = ctypes.c_int(0)

# name -> (acceptable arguments, stream first; [(1-based index, bad value), ...])
CASES = {
    "tg_syrk_accum": ([None, P, 2, 4, 8, 8, P, 8],
                      [(2, None), (3, 7), (4, -1), (5, 0), (6, 7), (7, None), (8, 7)]),
    "tg_syrk_accum_ws": ([None, P, 0, 4, 8, 8, P, 8, P, BIG],
                         [(2, None), (3, -1), (4, -1), (5, 0), (6, 7), (7, None), (8, 7)]),
    "tg_scale_f64": ([None, P, 10, 0.5, P], [(2, None), (3, -1), (5, None)]),
    "tg_sketch_omega": ([None, 1, 0, 4, 8, P, 8], [(3, -1), (4, 0), (5, -1), (6, None), (7, 7)]),
    "tg_sketch_accum": ([None, P, 2, 4, 8, 8, 1, 0, P, 4, 8],
                        [(2, None), (3, 3), (5, 0), (6, 7), (9, None), (10, 0), (11, 7)]),
    "tg_dgemm": ([None, 0, 0, 4, 5, 6, 1.0, P, 6, P, 5, 0.0, P, 5],
                 [(4, -1), (8, None), (9, 5), (11, 4), (14, 4)]),
    "tg_dgemm/tt": ([None, 1, 1, 4, 5, 6, 1.0, P, 4, P, 6, 0.0, P, 5],
                    [(9, 3), (11, 5), (14, 4)]),
    "tg_eigh_values": ([None, P, 8, 8, P, P, BIG], [(2, None), (3, 0), (4, 7), (5, None)]),
    "tg_eigh_vectors": ([None, 8, P, 4, P, 8, P, BIG],
                        [(2, 0), (3, None), (4, 0), (4, 9), (5, None), (6, 7)]),
    "tg_eigh_vectors_range": ([None, 8, P, 2, 4, P, 8, P, BIG],
                              [(2, 0), (3, None), (4, -1), (4, 8), (5, 0), (5, 7), (6, None),
                               (7, 7)]),
    "tg_band_tridiag": ([None, P, 40, 40, P, P, P, BIG],
                        [(2, None), (3, 0), (4, 39), (5, None), (6, None)]),
    "tg_truncation_rank": ([None, P, 8, 1e-4, 1, P, P],
                           [(2, None), (3, 0), (5, 3), (5, -1), (6, None), (7, None)]),
    "tg_pivoted_factor": ([None, P, 8, P, 8, 5, P, P, 8, P, BIG],
                          [(2, None), (3, 7), (4, None), (5, 0), (6, 0), (6, 9), (7, None),
                           (9, 7)]),
    "tg_u_factor": ([None, P, 8, P, P, 8, 5, P, 8, P, BIG],
                    [(2, None), (3, 7), (4, None), (5, None), (6, 0), (7, 0), (7, 9), (8, None),
                     (9, 7)]),
    "tg_qr_r": ([None, P, 8, 5, 8, P, BIG],
                [(2, None), (3, 7), (4, 0), (4, 9), (5, 0), (6, None)]),
    "tg_pivoted_factor_complement": ([None, P, 8, P, 8, P, 2, 8, 5, P, P, 8, P, BIG],
                                     [(2, None), (3, 7), (4, None), (5, 7), (6, None), (7, -1),
                                      (7, 4), (8, 0), (9, 0), (9, 9), (10, None), (12, 7)]),
    "tg_u_factor_rx": ([None, P, 8, 8, 5, P, 8, P, BIG],
                       [(2, None), (3, 7), (4, 0), (5, 0), (5, 9), (6, None), (7, 7)]),
    "tg_urx_c": ([None, P, 8, 8, 5, 0, 3, P, 3, P, BIG],
                 [(2, None), (3, 7), (5, 0), (5, 9), (6, -1), (6, 4), (7, 4), (8, None), (9, 2)]),
    "tg_urx_u11": ([None, P, 8, 8, 5, P, 3, P, 8, P, BIG],
                   [(2, None), (3, 7), (5, 0), (5, 9), (6, None), (7, 2), (8, None), (9, 7)]),
    "tg_urx_u12": ([None, P, 5, 5, P, 3, 3, P, 3],
                   [(2, None), (3, 4), (4, 0), (5, None), (6, 2), (7, -1), (8, None), (9, 2)]),
    "tg_pred_error": ([None, P, P, 4, 8, 8, P, 5, 8, P, P, P, BIG],
                      [(2, None), (3, None), (4, 0), (5, 0), (6, 7), (7, None), (8, 0), (9, 7),
                       (10, None), (11, None)]),
    "tg_group_params": ([None, P, 4, 8, 8, 4, 4, 0, P, P],
                        [(2, None), (3, 0), (4, 0), (5, 7), (6, 3), (7, 1), (7, 9), (9, None),
                         (10, None)]),
    "tg_process_block": ([None, P, 8, P, 8, P, 8, P, 8, 4, 8, 0, 15, P, 8, P, 8, P, BIG],
                         [(2, None), (3, 7), (4, None), (5, 7), (6, None), (7, 7), (8, None),
                          (9, 7), (10, 0), (11, 0), (11, 2049), (14, None), (15, 7), (16, None),
                          (17, 7)]),
    "tg_gptq_quantize": ([None, P, 4, 8, P, 5, 8, P, P, P, 4, 4, 0, 4, P, P, P, BIG],
                         [(2, None), (3, 0), (4, 0), (5, None), (6, 0), (6, 9), (7, 7), (8, None),
                          (9, None), (10, None), (11, 3), (12, 1), (12, 9), (14, 0), (14, 2049),
                          (15, None)]),
    "tg_hinv_chol": ([None, P, 8, 8, None, 0.01, 5, P, 8, ctypes.pointer(TRIES), P, BIG],
                     [(2, None), (3, 0), (4, 7), (7, 0), (8, None), (9, 7), (10, None)]),
    # the packed layout exists for 2, 3, 4 and 8 bits only (n * b = 160, 192, 224
    # are multiples of 32, so 5..7 are refused as widths, not through the size)
    "tg_pack_codes": ([None, P, 4, 32, 4, P],
                      [(2, None), (3, 0), (4, 0), (4, 33), (5, 1), (5, 5), (5, 6), (5, 7), (5, 9),
                       (6, None)]),
    "tg_pack_zeros": ([None, P, 32, 2, 4, 0, P],
                      [(2, None), (3, 0), (3, 33), (4, 0), (5, 1), (5, 5), (5, 6), (5, 7), (5, 9),
                       (7, None)]),
    "tg_dequant_packed": ([None, P, P, P, 0, 32, 64, 32, 4, P, 0, 64],
                          [(2, None), (9, 5), (10, None), (12, 63)]),
    "tg_qgemm": ([None, P, 0, 2, 64, P, P, P, 0, 32, 64, 32, 4, None, 0, P, 0, 32, P, BIG],
                 [(2, None), (5, 63), (13, 5), (16, None), (18, 31)]),
}
CASES["tg_gptq_quantize_loop"] = CASES["tg_gptq_quantize"]


class Spec(ctypes.c_int64 * 12):
    """A ChunkSpec for tg_gemm64_chunked (c, nc, m, six offsets, M, N, K) that
    prints as its values, so the test ids do not carry an address."""

    def __str__(self):
        return "spec" + "_".join(str(v) for v in self)


def spec(c=4, nc=2, m=8, M=3, N=5, K=6):
    return Spec(c, nc, m, 0, 0, 0, 0, 0, 0, M, N, K)


# the test hooks onto the internal FP64 GEMM family: op 0 / 1 / 2 take A (M x K),
# B (K x N) like tg_dgemm, op 3 sums nz slices, ops 4..7 are SYRKs of X = A
CASES.update({
    "tg_gemm64_probe": ([None, 0, 0, 0, 4, 5, 6, 1.0, P, 6, P, 5, 0.0, P, 5, 1, None, 0],
                        [(2, -1), (2, 8), (5, -1), (6, -1), (7, -1), (9, None), (10, 5),
                         (11, None), (12, 4), (14, None), (15, 4)]),
    "tg_gemm64_probe/tt": ([None, 0, 1, 1, 4, 5, 6, 1.0, P, 4, P, 6, 0.0, P, 5, 1, None, 0],
                           [(10, 3), (12, 5)]),
    "tg_gemm64_probe/upper_a": ([None, 1, 0, 0, 4, 5, 6, 1.0, P, 6, P, 5, 0.0, P, 5, 1, None, 0],
                                [(3, 1), (4, 1), (10, 5), (12, 4), (15, 4)]),
    "tg_gemm64_probe/splitk": ([None, 2, 0, 0, 4, 5, 6, 1.0, P, 6, P, 5, 0.0, P, 5, 2, P, BIG],
                               [(10, 5), (12, 4), (15, 4), (16, 0), (17, None),
                                (18, 4 * 5 * 2 * 8 - 1)]),
    "tg_gemm64_probe/sum_partials": ([None, 3, 0, 0, 4, 5, 0, 1.0, P, 0, None, 0, 0.0, P, 5, 2,
                                      None, 0],
                                     [(5, -1), (6, -1), (9, None), (14, None), (15, 4), (16, 0)]),
    "tg_gemm64_probe/syrk_tn": ([None, 4, 0, 0, 0, 5, 6, 1.0, P, 5, None, 0, 0.0, P, 5, 0, None, 0],
                                [(6, -1), (7, -1), (9, None), (10, 4), (14, None), (15, 4)]),
    "tg_gemm64_probe/syrk_tn_upper": ([None, 5, 0, 0, 0, 5, 0, 1.0, P, 5, None, 0, 0.0, P, 5, 0,
                                       None, 0], [(10, 4), (15, 4)]),
    "tg_gemm64_probe/syrk_tn_lower": ([None, 6, 0, 0, 0, 5, 6, 1.0, P, 5, None, 0, 0.0, P, 5, 0,
                                       None, 0], [(10, 4), (15, 4)]),
    "tg_gemm64_probe/syrk_nt": ([None, 7, 0, 0, 0, 5, 6, 1.0, P, 6, None, 0, 0.0, P, 5, 0, None, 0],
                                [(10, 5), (15, 4)]),
    "tg_gemm64_chunked": ([None, 0, 0, spec(), 0, 1.0, P, 6, P, 5, 0.0, P, 5],
                          [(4, None), (4, spec(c=0)), (4, spec(nc=-1)), (4, spec(m=-1)),
                           (4, spec(nc=4)), (4, spec(M=1 << 31)), (5, -1), (5, 3), (7, None),
                           (8, 5), (9, None), (10, 4), (12, None), (13, 4)]),
    # M / N / K < 0 stand for the longest chunk: c = 4, nc = 2, m = 11 -> 7
    "tg_gemm64_chunked/k": ([None, 0, 0, spec(m=11, K=-1), 0, 1.0, P, 7, P, 5, 0.0, P, 5],
                            [(8, 6)]),
    "tg_gemm64_chunked/tt": ([None, 1, 1, spec(m=11, M=-1), 0, 1.0, P, 7, P, 6, 0.0, P, 5],
                             [(8, 6), (10, 5)]),
    "tg_gemm64_chunked/n": ([None, 0, 0, spec(m=11, N=-1), 0, 1.0, P, 6, P, 7, 0.0, P, 7],
                            [(10, 6), (13, 6)]),
    "tg_gemm64_chunked/tri": ([None, 0, 0, spec(), 1, 1.0, P, 6, P, 5, 0.0, P, 5],
                              [(2, 1), (3, 1), (4, spec(M=0)), (8, 5)]),
})

PARAMS = [pytest.param(name, idx, bad, id=f"{name}-arg{idx}-{bad}")
          for name, (_, bads) in CASES.items() for idx, bad in bads]


@pytest.mark.parametrize("name,idx,bad", PARAMS)
def test_bad_argument_is_rejected_with_its_index(L, name, idx, bad):
    base, _ = CASES[name]
    args = list(base)
    args[idx - 1] = bad
    fn = getattr(L.lib, name.split("/")[0])
    rc = fn(*args)
    msg = L.last_error()
    assert rc == -idx, (rc, msg)
    assert f"argument {idx}:" in msg, msg


def test_every_entry_point_with_a_leading_dimension_is_covered():
    """The table above has a case for every `ld*` parameter the header declares."""
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "truncgptq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    missing = []
    for name, params in re.findall(r"\bint (tg_[a-z0-9_]+)\s*\(([^)]*)\)", src):
        names = [p.split()[-1].lstrip("*") for p in params.split(",") if p.strip() != "void"]
        tested = {i for key, (_, bads) in CASES.items() if key.split("/")[0] == name
                  for i, _ in bads}
        for pos, pname in enumerate(names, start=1):
            if re.fullmatch(r"ld[a-z0-9]*", pname) and pos not in tested:
                missing.append((name, pname))
    assert not missing, missing
