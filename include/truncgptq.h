/* truncgptq.h -- C ABI of the MI355X-native TruncGPTQ per-layer solver.
 *
 * Every entry point takes plain device pointers, explicit sizes / leading
 * dimensions (row-major, element units) and the caller's hipStream_t
 * (passed as void* so this header needs no HIP include).  Work is
 * stream-ordered; nothing here synchronises the device unless the comment
 * says so.  Scratch memory comes from the caller (`ws`, `ws_bytes`), sized
 * by the matching *_workspace_size() query; the library allocates nothing.
 *
 * A leading dimension may exceed the width, and a matrix pointer needs only
 * the alignment of its element type (it may point into the middle of an
 * allocation): 16-byte loads are taken only where the pointer and the leading
 * dimension allow them, 8- / 4-byte loads otherwise.  (One exception, by
 * design: from trailing widths of 6144 up, tg_eigh_values reads pairs of
 * adjacent columns of A with one 16-byte load that is only 8-byte aligned when
 * the width or lda is odd; gfx950 global loads permit that.)  Nothing outside the
 * logical matrix of an output (the columns width .. ld-1 included) is written,
 * and inputs declared const are left unchanged.  A leading dimension below
 * the width, a null pointer or a size out of range is rejected with that
 * argument's index before any device work (tests/test_abi_args.py).
 *
 * Return value: 0 ok; <0 invalid argument (-(1-based argument index));
 * >0 a hipError_t.  tg_last_error() returns a thread-local message.
 *
 * Reference = /root/reference/src/TruncGPTQ (davidtweedle/gptq-svd).
 */
#ifndef TRUNCGPTQ_H
#define TRUNCGPTQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- misc --------------------------------------------------------------- */
const char *tg_last_error(void);
int tg_version(void);

/* Sampled HIP-event timing of the hot kernel classes (for bench roofline
 * reporting).  Classes: 0 tri_symv, 1 cross_gemm, 2 quant_block, 3 tri_syr2k,
 * 4 pivot_step, 5 bisect, 6 inverse_iteration, 7 back_transform, 8 bulge_chase,
 * 9 tsqr_leaf (the panel QR kernels), 10 band_update, 11 q1_apply, 12 q2_apply
 * (the order of PROF_CLASSES in gptq-svd_amd/_lib.py).
 * tg_profile_query synchronises on the recorded events. */
int tg_profile_enable(int on, int every);
int tg_profile_reset(void);
int tg_profile_query(int id, double *ms, int64_t *sampled, double *bytes, double *flops,
                     int64_t *total_launches);

enum tg_dtype { TG_F16 = 0, TG_BF16 = 1, TG_F32 = 2, TG_F64 = 3 };
enum tg_rank_rule { TG_RULE_NONE = 0, TG_RULE_ENERGY = 1, TG_RULE_MEAN_TRIMMED = 2 };

/* ---- A1: Hessian accumulation -------------------------------------------
 * Replaces HessianAccumulator.add_batch: `self.H.addmm_(x.T, x)` after the
 * cast to float64 (gptq_utils.py:218-223).  H (n x n, ld ldh) += X^T X where
 * X is (rows x n, ld ldx) of dtype x_dtype (products formed in float64).
 * Both triangles of H are written (the reference keeps the full matrix). */
int tg_syrk_accum(void *stream, const void *X, int x_dtype, int64_t rows, int n, int64_t ldx,
                  double *H, int ldh);

/* The same update with a caller workspace (tg_syrk_workspace_size(n) bytes,
 * independent of rows: the partial tiles of the last round of 128 x 128 tiles,
 * Tt = min(tiles, resident workgroups) tiles x 16 chunks x 128 KiB, i.e. about
 * 1 GiB on a 256-CU MI355X once n >= ~4000): fp16 / bf16 X with n and ldx
 * multiples of 8 and a 16-byte aligned X take the dedicated 16-bit SYRK
 * (syrk.hip: X kept 16-bit in LDS, lower 128 x 128 tiles handed out by an
 * atomic queue over a static decomposition whose partial tiles are summed in
 * a fixed order -- deterministic); other inputs fall back to tg_syrk_accum. */
size_t tg_syrk_workspace_size(int n);
int tg_syrk_accum_ws(void *stream, const void *X, int x_dtype, int64_t rows, int n, int64_t ldx,
                     double *H, int ldh, void *ws, size_t ws_bytes);

/* Replaces HessianAccumulator.get_hessian `self.H / self.n_samples`
 * (gptq_utils.py:225-228).  inv_n > 0: out = H * inv_n; inv_n < 0:
 * out = H / (-inv_n) (exact true division, the reference's semantics).
 * out may alias H. */
int tg_scale_f64(void *stream, const double *H, int64_t count, double inv_n, double *out);

/* ---- A1s: Gaussian sketch accumulation -----------------------------------
 * Replaces Sketcher.hook_fn (gptq_utils.py:184-202): `R = torch.randn(rank,
 * tokens)` followed by `Y.addmm_(R, x.float())`.  Here Omega is generated
 * inside the GEMM kernel and never stored.  Contract:
 *
 * omega is a pure function of (seed, r, g), r the sketch row and g = t0 + t
 * the global token index; nothing else (tile, launch shape, rank, T) enters.
 *   Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 *   (g & 0xffffffff, g >> 32, (r >> 7) * 32 + (r & 31), 0).  Its outputs
 *   x0..x3 serve the four rows that differ only in j = (r >> 5) & 3, by
 *   Box-Muller on the pairs (x0, x1) -> j = 0, 1 and (x2, x3) -> j = 2, 3:
 *   u1 = ((xa >> 8) + 1) * 2^-24 in (0, 1] (the log never sees 0),
 *   u2 = (xb >> 8) * 2^-24 in [0, 1), rad = sqrtf(-2 logf(u1)),
 *   omega = rad * cos(2 pi u2) for the even j, rad * sin(2 pi u2) for the odd
 *   (fp32; cospif / sinpif of the exact 2 u2).
 * tg_sketch_omega and tg_sketch_accum call the same device function, so the
 * values they use are bit-identical.
 *
 * Each Y[r, c] is one fp32 fused-multiply-add chain in ascending t that starts
 * from the value already in Y:
 *   acc = Y[r, c];  acc = fmaf(omega(seed, r, t0 + t), float(X[t, c]), acc),
 *   t = 0 .. T-1
 * (v_mfma_f32_32x32x2_f32 with the accumulator loaded from Y; the conversion
 * of X to fp32 is exact).  No split over tokens, no atomics, no workspace; K
 * padding multiplies zero by zero.  Hence, bitwise: one call over T tokens
 * equals any split of the same tokens into consecutive calls with advancing
 * t0, and rows 0..r1-1 of a rank-r2 sketch equal the rank-r1 sketch.
 * Columns n .. ldy-1 of Y are not touched.
 *
 * Omega[r][t] (rank x T fp32, ld ldo) = omega(seed, r, t0 + t).  Tests / tools
 * only (rank <= 65535). */
int tg_sketch_omega(void *stream, uint64_t seed, int64_t t0, int rank, int64_t T,
                    float *Omega, int64_t ldo);
/* Y (rank x n fp32, ld ldy) += Omega(seed; rows 0..rank-1, tokens t0..t0+T-1) * X,
 * X (T x n, ld ldx) of x_dtype TG_F16 / TG_BF16 / TG_F32.  T = 0 is a no-op.
 * Limits (rejected with the argument index): ldy < 2^21, because a workgroup
 * addresses its 512-row tile of Y with 32-bit offsets (-11); rank <= 65535 *
 * 512 (-10); t0 >= 0 and t0 + T <= INT64_MAX (-8, -4). */
int tg_sketch_accum(void *stream, const void *X, int x_dtype, int64_t T, int n, int64_t ldx,
                    uint64_t seed, int64_t t0, float *Y, int rank, int64_t ldy);

/* FP64 MFMA GEMM used by every dense stage (exported for tests / reuse):
 * C = alpha op(A) op(B) + beta C, row-major, op(A) M x K, op(B) K x N.
 * Hand-written kernels only (gemm64.hip: 8-wave 128 x 128 tiles for large
 * products, 64 x 64 tiles otherwise); no vendor BLAS is linked.  lda / ldb are
 * those of A / B as stored (K x M when transA, N x K when transB). */
int tg_dgemm(void *stream, int transA, int transB, int M, int N, int K, double alpha,
             const double *A, int lda, const double *B, int ldb, double beta, double *C, int ldc);

/* The rest of the internal FP64 GEMM family (gemm64.h), one switch onto the
 * functions the dense stages call.  Tests / tools only; product code does not
 * come through here.  Stream-ordered, synchronises nothing.  Row-major, C (ld
 * ldc) updated in place as C = alpha * (product) + beta * C; with beta == 0, C
 * is not read.  Per op:
 *   TG_G64_GEMM          dgemm, the arguments of tg_dgemm;
 *   TG_G64_UPPER_A       dgemm_upper_a: C = alpha A B + beta C with A (M x K,
 *                        M <= K) upper triangular; of A's zeros only those in
 *                        the tile rows' own diagonal blocks are read (the sum
 *                        of the tile row starting at tm begins at k = tm);
 *                        transA = transB = 0;
 *   TG_G64_SPLITK        dgemm_splitk over `splits` K ranges; ws holds
 *                        tg_gemm64_probe_workspace_size(op, M, N, splits) bytes
 *                        (M * N * splits doubles, written before they are read);
 *   TG_G64_SUM_PARTIALS  sum_partials: C (M x N) = alpha sum_z P_z + beta C,
 *                        A = P (splits = nz >= 1 slices of M x N, ld N);
 *   TG_G64_SYRK_TN       dsyrk_tn: C (n x n) = alpha X^T X + beta C, X (K x n),
 *                        lower tiles computed and mirrored: C is exactly
 *                        symmetric when beta C was;
 *   TG_G64_SYRK_TN_UPPER dsyrk_tn_upper: the same for an upper-triangular X
 *                        (n x n, strict lower triangle exactly 0; K ignored);
 *   TG_G64_SYRK_TN_LOWER dsyrk_tn_lower: the 64 x 64 lower and diagonal tiles
 *                        only; the strict upper triangle outside the diagonal
 *                        tiles is not written;
 *   TG_G64_SYRK_NT       dsyrk_nt: C (n x n) = alpha X X^T + beta C, X (n x K).
 * For the SYRK ops N is n, A is X and lda is ldx; M, B, ldb, transA and transB
 * are ignored (B may be NULL).  SUM_PARTIALS ignores lda, B, ldb, K.  Only
 * SPLITK takes a workspace; every other op needs 0 bytes (ws may be NULL). */
enum tg_gemm64_op { TG_G64_GEMM = 0, TG_G64_UPPER_A = 1, TG_G64_SPLITK = 2,
                    TG_G64_SUM_PARTIALS = 3, TG_G64_SYRK_TN = 4, TG_G64_SYRK_TN_UPPER = 5,
                    TG_G64_SYRK_TN_LOWER = 6, TG_G64_SYRK_NT = 7 };
size_t tg_gemm64_probe_workspace_size(int op, int M, int N, int splits);
int tg_gemm64_probe(void *stream, int op, int transA, int transB, int M, int N, int K,
                    double alpha, const double *A, int lda, const double *B, int ldb,
                    double beta, double *C, int ldc, int splits, void *ws, size_t ws_bytes);
/* dgemm_chunked (gemm64.h), the grouped GEMM of the band reduction and the
 * triangular inverse.  Tests / tools only; synchronises nothing.  spec (host
 * memory, read during the call) holds the 12 fields of ChunkSpec in order:
 * c, nc, m, a_kb, a_z, b_kb, b_z, c_kb, c_z, M, N, K.  Chunk z = 0 .. nc-1
 * covers [kb, ke) of a length-m axis, kb = z c, ke = m for the last chunk and
 * kb + c otherwise, and computes C_z = alpha op(A_z) op(B_z) + beta C_z with
 * X_z = X + kb x_kb + z x_z (element offsets) and M / N / K the given value or,
 * when negative, the chunk length ke - kb.  Needs c > 0, nc >= 0, m >= (nc-1) c
 * and lda / ldb / ldc at least the widths of one chunk's operands as stored;
 * keeping the chunks inside the caller's buffers is the caller's business.
 * tri = 1: every A_z is upper triangular, tri = 2: every B_z (K x N) is; the
 * zero triangle is skipped per tile, so of its zeros only those in the tiles'
 * diagonal blocks are read.  tri != 0 takes no transposes and M, N >= 1. */
int tg_gemm64_chunked(void *stream, int transA, int transB, const int64_t *spec, int tri,
                      double alpha, const double *A, int lda, const double *B, int ldb,
                      double beta, double *C, int ldc);

/* ---- A2: symmetric eigensolver (torch.linalg.eigh, gptq_utils.py:93) ----
 * Stage 1: A (n x n symmetric, full storage, destroyed) -> tridiagonal
 * (Householder, lower) + all eigenvalues ascending in w_asc (n).  The
 * reflectors stay in ws for stage 2. */
size_t tg_eigh_workspace_size(int n);
int tg_eigh_values(void *stream, double *A, int n, int lda, double *w_asc, void *ws,
                   size_t ws_bytes);
/* Stage 2: eigenvectors of the `k` LARGEST eigenvalues, in DESCENDING order,
 * written as ROWS of Vh (k x n, ld ldv) -- i.e. the reference's
 * `V.T.flip(0)[:k]` (gptq_utils.py:95,110).  Uses the stage-1 workspace. */
int tg_eigh_vectors(void *stream, int n, const double *w_asc, int k, double *Vh, int ldv,
                    void *ws, size_t ws_bytes);
/* Eigenvectors of the eigenvalues first .. first+count-1 in DESCENDING
 * order (rows of Vh, count x n).  tg_eigh_vectors(k) = range(0, k).  The
 * complement path below asks for the dropped eigenpairs k .. k+nc-1. */
int tg_eigh_vectors_range(void *stream, int n, const double *w_asc, int first, int count,
                          double *Vh, int ldv, void *ws, size_t ws_bytes);
/* The band -> tridiagonal stage of tg_eigh_values on its own (tests, tools):
 * A (n x n, full storage, ld lda) holds a symmetric band matrix of
 * half-bandwidth 32 (only the lower band A[c + d][c], d <= 32, is read);
 * on return d (n) / e (n - 1 used) hold a similar symmetric tridiagonal.
 * Bulge chasing as in tg_eigh_values (part of the eigh of
 * gptq_utils.py:93).  Synchronises the stream (reads the stall word);
 * a stalled hand-off returns hipErrorLaunchTimeOut. */
size_t tg_band_tridiag_workspace_size(int n);
int tg_band_tridiag(void *stream, const double *A, int n, int lda, double *d, double *e, void *ws,
                    size_t ws_bytes);

/* ---- A3: truncation rank (gptq_utils.py:97-108) ---------------------------
 * From ascending eigenvalues: S = sqrt(max(L, 1e-12)) descending, then the
 * rank rule.  Writes S_desc (n) and k (int32, device) -- no host sync.
 * `rule` is a tg_rank_rule; any other value is rejected (-5). */
int tg_truncation_rank(void *stream, const double *w_asc, int n, double threshold, int rule,
                       double *S_desc, int32_t *k_dev);

/* ---- A4: pivot order + R_x (jax.scipy.linalg.qr(pivoting=True) on
 * S_k = diag(S) Vh_k, gptq_utils.py:112-117, 122-123) -----------------------
 * Computes the dgeqp3 column order `perm` (n, int64) and the sign-normalised
 * R_x (k x n upper trapezoidal, ld ldr; may be NULL).  Algorithm: greedy
 * diagonal pivoting on H_k = S_k^T S_k (identical pivot rule to dgeqp3; see
 * DESIGN.md). */
size_t tg_pivot_workspace_size(int n, int k);
int tg_pivoted_factor(void *stream, const double *Vh, int ldv, const double *S, int n, int k,
                      int64_t *perm, double *Rx, int ldr, void *ws, size_t ws_bytes);

/* ---- A5: U = sign-normalised R of QR(diag(1/S) Vh_k[:, perm])
 * (gptq_utils.py:111, 118-124).  U (k x n, ld ldu) upper trapezoidal with
 * positive diagonal; U^T U = P^T H_k^+ P. */
size_t tg_ufactor_workspace_size(int n, int k);
int tg_u_factor(void *stream, const double *Vh, int ldv, const double *S, const int64_t *perm,
                int n, int k, double *U, int ldu, void *ws, size_t ws_bytes);

/* Which factor the calling thread's last tg_u_factor / tg_u_factor_rx /
 * tg_urx_u11 call returned: 0 the Gram-form (Cholesky) factor, 1 the Gram form
 * with CholeskyQR refinement, 2 the Householder QR below.  The Gram form
 * squares the condition number; when its shifted CholeskyQR3 refinement breaks
 * down, the factor is taken from a Householder QR instead, as the reference
 * does throughout (gptq_utils.py:120).  TG_U_QR (read per call) = auto
 * (default) | gram (no fallback: the breakdown is returned as an error) |
 * householder (no Gram attempt). */
int tg_u_factor_last_path(void);

/* Blocked Householder QR, R only (the QR of gptq_utils.py:120 without Q):
 * A (k x n row-major, 1 <= k <= n, ld lda >= n) becomes its upper-trapezoidal
 * R in place: strict lower triangle exactly 0, rows sign-flipped so the
 * diagonal is >= 0, columns n .. lda-1 untouched.  Communication-avoiding
 * (TSQR-tree) panels of 32 columns, trailing update by FP64 MFMA (hqr.hip);
 * deterministic.  Column norms are scaled (as dnrm2), so squares neither
 * overflow nor underflow.  Synchronises the stream once, at the end, to read
 * the breakdown word: a non-finite column norm, or a non-finite entry of the
 * finished R (which a NaN / Inf anywhere in A leaves), returns hipErrorUnknown
 * with a "broke down" message. */
size_t tg_qr_r_workspace_size(int k, int n);
int tg_qr_r(void *stream, double *A, int lda, int k, int n, void *ws, size_t ws_bytes);

/* ---- A4/A5 complement path (same outputs, no kept eigenvectors) ----------
 * When the dropped eigenpairs above rounding level are fewer than the kept
 * ones (k > n/2, the usual case: Qwen3-8B keeps ~99.5%), H_k = H - B_c^T B_c
 * with B_c = diag(S_c) Vc (Vc: nc x n rows = eigenvectors k .. k+nc-1 in
 * descending order from tg_eigh_vectors_range, S_c = S_desc[k:k+nc]); the
 * pivot order and R_x come from the same greedy pivoting as
 * tg_pivoted_factor (workspace: tg_pivot_workspace_size(n, k)), and U from
 * R_x alone: U = R(QR(S^-1 R_x)), S = R_x R_x^T. */
int tg_pivoted_factor_complement(void *stream, const double *H, int ldh, const double *Vc,
                                 int ldvc, const double *Sc, int nc, int n, int k, int64_t *perm,
                                 double *Rx, int ldr, void *ws, size_t ws_bytes);
size_t tg_ufactor_rx_workspace_size(int n, int k);
int tg_u_factor_rx(void *stream, const double *Rx, int ldr, int n, int k, double *U, int ldu,
                   void *ws, size_t ws_bytes);

/* The same U factor (explicit form: m = n - k > k / 16) in column-sharded
 * pieces for one process per GPU (gptq_svd_amd.dist.u_factor_rx_sharded; no
 * reference counterpart: the reference is single-device, quantize.py:180-184).
 * C = R11^-1 R12 (R11 = Rx[:, :k], R12 = Rx[:, k:]):
 *   tg_urx_c:   C[:, c0:c1] into C (k x (c1 - c0), ld ldc);
 *   tg_urx_u11: U[:, :k] = V^-1 from the whole C (k x (n - k), ld ldc);
 *   tg_urx_u12: out (k x ncols, ld ldo) = U[:, :k] C_block.
 * Each entry of C and U12 depends on its own column only, so gathering the
 * ranks' blocks gives tg_u_factor_rx's U bit for bit.  Workspace:
 * tg_ufactor_rx_workspace_size(n, k) for tg_urx_c / tg_urx_u11. */
int tg_urx_c(void *stream, const double *Rx, int ldr, int n, int k, int c0, int c1, double *C,
             int ldc, void *ws, size_t ws_bytes);
int tg_urx_u11(void *stream, const double *Rx, int ldr, int n, int k, const double *C, int ldc,
               double *U, int ldu, void *ws, size_t ws_bytes);
int tg_urx_u12(void *stream, const double *U, int ldu, int k, const double *C, int ldc, int ncols,
               double *out, int ldo);

/* ---- A6: relative prediction error (log_quantization_error,
 * gptq_utils.py:275-291) ---------------------------------------------------
 * out[0] = ||W[:, perm] R^T||_F^2, out[1] = ||(W - Wq)[:, perm] R^T||_F^2
 * (device, 2 doubles) with R = R_x (k x n, ld ldr) rounded to float32, the
 * reference's `R_x.to(float32)`.  W, Wq: m x n float32 (ld ldw), original
 * column order; perm: n int64.  The products are FP32 MFMA (TF32 off in the
 * reference), the sums of squares FP64; the caller takes sqrt(out[1] / out[0]). */
size_t tg_pred_error_workspace_size(int m, int n, int k);
int tg_pred_error(void *stream, const float *W, const float *Wq, int m, int n, int ldw,
                  const double *Rx, int k, int ldr, const int64_t *perm, double *out, void *ws,
                  size_t ws_bytes);

/* ---- A7: Quantizer.find_params (gptq_utils.py:249-266) --------------------
 * W (m x n f32, ld ldw) -> scale, zero (m x n/g f32, ld n/g); g = group, or n
 * when group <= 0.  Any g >= 1 that divides n is served, g = 1 and groups
 * narrower than a wave included. */
int tg_group_params(void *stream, const float *W, int m, int n, int ldw, int group, int w_bits,
                    int sym, float *scale, float *zero);

/* ---- A7c: Hessian-weighted clip search for scale / zero (new; candidate 0
 * is find_params, gptq_utils.py:249-266) ----------------------------------
 * W (m x n f32, row stride stride_w >= n), groups of g consecutive original
 * columns (g = group, or n when group <= 0; any g >= 1 dividing n),
 * col_weight = h (n f32 >= 0; null = all ones), maxq / minq as in Quantizer,
 * grid >= 1, 0 <= steps < grid.  Candidates i = 0 .. steps with
 * p = 1.0f - float(i) / float(grid); every f32 operation below is one
 * correctly rounded operation in the order written, no contraction, true
 * division.
 *   asym (mn, mx the group's min, max):
 *     lo = mn < 0 ? p * mn : mn;  hi = mx > 0 ? p * mx : mx;
 *     d = max(hi - lo, 1e-5f);  s = d / maxq;  z = clamp(rintf(-lo / s), 0, maxq)
 *   sym (a the group's max |w|):  s = max(p * a, 1e-5f) / maxq;  z = 0
 *   objective over the group's elements c (the tail / RTN rounding rule,
 *   gptq_utils.py:552-553):
 *     q = clamp(rintf(w_c / s + z), minq, maxq);  dq = (q - z) * s;  e = w_c - dq
 *     J_i = sum_c double(h_c) * (double(e) * double(e)), summed in fp64 in an
 *     order that is the same for every candidate and every call (no atomics).
 * Chosen: the smallest i with minimal J_i (only a strictly smaller J replaces
 * the best so far).  Candidate 0 is tg_group_params, so steps = 0 reproduces
 * it bit for bit, and J_chosen <= J_0 always.
 * Outputs: scale, zero (m x n/g f32, laid out as tg_group_params writes
 * them); choice (nullable, m x n/g int32: the chosen i); objective (nullable,
 * m x n/g x 2 doubles: {J_0, J_chosen}).  No workspace. */
int tg_group_params_clip(void *stream, const float *W, int m, int n, int64_t stride_w,
                         const float *col_weight, int group, int w_bits, int sym, int grid,
                         int steps, float *scale, float *zero, int32_t *choice,
                         double *objective);

/* ---- A9: triton_process_block (gptq_utils.py:393-453, kernel :298-386) ----
 * One block: w, s, z (m x B f32, ld ldw/lds/ldz), R (B x B f32, ld ldr).
 * Outputs q (dequantised) and e (raw error), m x B, ld ldq / lde.  Each of the
 * six leading dimensions must be >= B (rejected with its own index: -3, -5,
 * -7, -9, -15, -17). */
size_t tg_process_block_workspace_size(int B);
int tg_process_block(void *stream, const float *w, int ldw, const float *s, int lds,
                     const float *z, int ldz, const float *R, int ldr, int m, int B, int minq,
                     int maxq, float *q, int ldq, float *e, int lde, void *ws, size_t ws_bytes);

/* ---- A8-A12: gptq_fwrd(use_triton=True) (gptq_utils.py:459-565) ---------
 * W (m x n f32, original column order), U (k x n f32, ld ldu), perm (n
 * int64), scale/zero from tg_group_params.  Writes Wq (m x n f32,
 * dequantised, original order) and codes (m x n uint8, original order,
 * stored +2^(b-1) when sym).  `block` is the reference's block_size. */
size_t tg_quantize_workspace_size(int m, int n, int block);
int tg_gptq_quantize(void *stream, const float *W, int m, int n, const float *U, int k, int ldu,
                     const int64_t *perm, const float *scale, const float *zero, int group,
                     int w_bits, int sym, int block, float *Wq, uint8_t *codes, void *ws,
                     size_t ws_bytes);

/* ---- §8(f) GPTQ comparator: gptq_fwrd(use_triton=False)
 * (gptq_utils.py:516-534 column loop, :544 cross-block GEMM) ---------------
 * Same arguments as tg_gptq_quantize; U is the comparator's H_inv_sqrt
 * (tg_hinv_chol).  Per column: q = clamp(round-half-even(w/s + z)),
 * err = (w - (q - z) s) / U[c, c], later block columns w_j -= err * U[c, j];
 * cross-block W[:, i2:] -= Err @ U[i1:i2, i2:] (k-ordered fmaf chain). */
int tg_gptq_quantize_loop(void *stream, const float *W, int m, int n, const float *U, int k,
                          int ldu, const int64_t *perm, const float *scale, const float *zero,
                          int group, int w_bits, int sym, int block, float *Wq, uint8_t *codes,
                          void *ws, size_t ws_bytes);

/* ---- §8(f) GPTQ comparator: process_hessian (gptq_utils.py:129-165) ------
 * R (n x n f64, ld ldr) = upper Cholesky factor of inv(H_p + damp I),
 * H_p = H[perm][:, perm] (perm may be NULL = identity; actorder's perm is
 * computed by the caller), damp = 10^e * damp_percent * mean(diag(H)) for
 * e = 0 .. max_tries-1 until H_p + damp I is positive definite (the
 * reference's ladder, :148-160).  *tries_used (host) = the rung e that
 * succeeded, or max_tries when every rung failed, in which case R = I (the
 * reference's intended fallback, :162-164).  Synchronises the stream once
 * per rung (the reference's try/except is a host round trip too). */
size_t tg_hinv_chol_workspace_size(int n);
int tg_hinv_chol(void *stream, const double *H, int n, int ldh, const int64_t *perm,
                 double damp_percent, int max_tries, double *R, int ldr, int *tries_used,
                 void *ws, size_t ws_bytes);

/* ---- A13: packing (absent in the reference; README.md:133) ----------------
 * codes (m x n uint8, offset form) -> qweight (n*b/32 x m int32, bit stream
 * along in_features; AutoGPTQ layout for b in {2,3,4,8}); zero (m x G f32)
 * -> qzeros (G x m*b/32 int32, stored zero + 2^(b-1) when sym).  Any other
 * w_bits (5, 6, 7 included) is rejected (-5), as tg_dequant_packed and tg_qgemm
 * reject it: no consumer reads such a stream. */
int tg_pack_codes(void *stream, const uint8_t *codes, int m, int n, int w_bits, int32_t *qweight);
int tg_pack_zeros(void *stream, const float *zero, int m, int G, int w_bits, int sym,
                  int32_t *qzeros);

/* ---- A14: packed inference (absent in the reference) ----------------------
 * The consumer of the A13 layout.  qweight int32 (n*b/32 x m): value i of
 * output feature r occupies bits [i*b, i*b+b) of the little-endian stream of
 * column r; qzeros int32 (G x m*b/32): the same stream along the output
 * features; scales (G x m) of scale_dtype TG_F16 or TG_F32; G = n/g with
 * g = group, or n when group <= 0; b in {2, 3, 4, 8}.  Codes and zeros are
 * stored in offset form, so sym and asym decode alike:
 * w = (code_u - zero_u) * scale.
 *
 * tg_dequant_packed: out (m x n, ld ldo, original column order) of out_dtype
 * TG_F16 / TG_BF16 / TG_F32.  Numerics: float(code_u - zero_u) * float(scale),
 * one fp32 multiply of an exact integer, then one round-to-nearest-even to
 * out_dtype, so a host computation reproduces it bit for bit.  Requires
 * (n*b) % 32 == 0, (m*b) % 32 == 0 and g dividing n. */
int tg_dequant_packed(void *stream, const int32_t *qweight, const int32_t *qzeros,
                      const void *scales, int scale_dtype, int m, int n, int group, int w_bits,
                      void *out, int out_dtype, int64_t ldo);

/* tg_qgemm: Y (T x m, ld ldy) = X (T x n, ld ldx) * W^T (+ bias), x_dtype
 * TG_F16 or TG_BF16, y_dtype = x_dtype or TG_F32, bias (m, nullable) of
 * bias_dtype TG_F16 / TG_BF16 / TG_F32.  Numerics: the weight operand is
 * exactly tg_dequant_packed's output with out_dtype = x_dtype; products and
 * sums are fp32; the bias is added in fp32; one rounding to y_dtype.  The
 * result is bit-identical from call to call (no atomics).
 * Requires n % 32 == 0, g % 32 == 0 and (m*b) % 32 == 0; anything else is
 * rejected with the argument index before any device work.
 * Two regimes.  gemv (T <= 16; chosen up to T = 4): 64 output features per
 * workgroup, K split over S workgroups of at most 512 values each.  mfma (any
 * T; chosen above): an MFMA tile kernel that unpacks 128-value K slabs of its
 * (64 or 128 rows) x 64 features tile into LDS; it splits K as well (S splits
 * of at least 512 values) while the output tiles alone are fewer than ~512
 * workgroups.  With S > 1 the partial sums [S][T][m] fp32 go to the workspace
 * and a second kernel adds them in ascending split order, then the bias; with
 * S = 1 the MFMA kernel writes Y itself.  The environment variable TG_QGEMM =
 * auto | gemv | mfma (read per call) forces a regime; gemv with T > 16 is an
 * argument error (-4).
 * tg_qgemm_workspace_size(T, m, n): S*T*m*4 bytes (+ alignment slack) for the
 * larger S of the regimes that take T (at m = n = 4096: S = 16 for T <= 16,
 * 8 at T = 64, and 0 bytes once the tiles fill the device, e.g. T = 4096). */
size_t tg_qgemm_workspace_size(int T, int m, int n);
int tg_qgemm(void *stream, const void *X, int x_dtype, int T, int64_t ldx, const int32_t *qweight,
             const int32_t *qzeros, const void *scales, int scale_dtype, int m, int n, int group,
             int w_bits, const void *bias, int bias_dtype, void *Y, int y_dtype, int64_t ldy,
             void *ws, size_t ws_bytes);

/* ---- A15: MXFP4 weight format (new; OCP Microscaling FP4) ------------------
 * E2M1 elements, one shared E8M0 power-of-two scale per 32 values.  `fmt` is a
 * tg_weight_format; TG_FMT_MXFP4 is its only value (anything else is rejected
 * with fmt's argument index).  Every f32 operation below is one correctly
 * rounded operation in the order written, no contraction.  Weights are finite;
 * NaN and Inf are outside the contract.
 *
 * Groups: 32 consecutive columns in the original column order, per row;
 * n % 32 == 0.  Static groups, gathered through perm like the integer scales.
 *
 * Scale (tg_group_params_mx; W m x n f32 with row stride stride_w >= n, both
 * outputs m x n/32): a = max |w| over the group; e = floor(log2 a),
 * the unbiased exponent (subnormals: their true floor(log2); a == 0: -inf);
 * E = max(e - 2, -126), 2 being E2M1's emax; E <= 125 for finite a.
 * scale = 2^E, always a normal f32; the stored byte is E + 127, in [1, 252]:
 * byte 255 (NaN) is never written.
 *
 * Element: t = w / scale, m = |t|,
 *   idx = (m > 0.25) + (m >= 0.75) + (m > 1.25) + (m >= 1.75) + (m > 2.5)
 *       + (m >= 3.5) + (m > 5)
 * indexes {0, 0.5, 1, 1.5, 2, 3, 4, 6}: round to nearest, ties to the even
 * code, saturating at 6.  code = idx | (8 if t < 0 and idx != 0 else 0): code 8
 * (-0) is never produced.  qv = +-grid[idx] * scale, +0 for idx == 0.  The
 * kernels multiply by the exactly representable 2^-E instead of dividing, which
 * is bit-identical.
 *
 * tg_gptq_quantize_mx: tg_gptq_quantize (loop = 0: err = w - qv) or
 * tg_gptq_quantize_loop (loop = 1: err = (w - qv) / U[c, c]) with the element
 * rule in place of the integer rule, in the column chain and in the tail beyond
 * rank k; everything else (separately rounded mul and sub in panel order, the
 * k-ordered fmaf chain across blocks, the unpermute) as there.  scale is
 * tg_group_params_mx's (m x n/32 f32), U is k x n with row stride stride_u;
 * codes (m x n uint8, values 0..15 except 8, original column order; nullable).
 * Workspace: tg_quantize_workspace_size.
 *
 * Packed image: qweight = tg_pack_codes(w_bits = 4) of those codes;
 * tg_pack_e8m0 transposes the scale bytes (m x G) into (G x m), which the
 * consumers read coalesced.
 *
 * Decode (tg_dequant_mx, and the weight operand of tg_qgemm_mx):
 * float(+-grid[code & 7]) * ldexpf(1, byte - 127), one f32 multiply, then one
 * round-to-nearest-even to the output / operand type.  Bytes 0 .. 254 all
 * decode (byte 0 is the subnormal 2^-127).  fp16 overflows to inf from 6 * 2^14
 * up (byte >= 141) and flushes small scales to zero; bf16 covers the range.
 * In fp32 the values 4 and 6 overflow from byte 253 up (6 * 2^125, byte 252, the
 * largest the solver writes, is finite).  out: m x n (row stride stride_o >= n),
 * out_dtype TG_F16 / TG_BF16 / TG_F32.  Requires n % 32 == 0 and
 * (m * 4) % 32 == 0.
 *
 * tg_qgemm_mx: tg_qgemm on that operand: Y (T x m) = X (T x n) * W^T (+ bias),
 * the weight operand exactly tg_dequant_mx's output in x_dtype, products and
 * sums f32, the bias added in f32, one rounding, bit-identical from call to
 * call.  The same two regimes, the same TG_QGEMM switch, the same workspace
 * (tg_qgemm_workspace_size) and the same argument checks as tg_qgemm; stride_x
 * >= n and stride_y >= m are the row strides of X and Y.
 * Weights only: activations stay 16-bit here; tg_qgemm_mx_act (A16, below) is
 * the opt-in W4A8 path on the block-scaled MFMA instructions, which need both
 * operands in low precision. */
enum tg_weight_format { TG_FMT_MXFP4 = 1 };
int tg_group_params_mx(void *stream, const float *W, int m, int n, int stride_w, int fmt,
                       float *scale, uint8_t *e8m0);
int tg_gptq_quantize_mx(void *stream, const float *W, int m, int n, const float *U, int k,
                        int stride_u, const int64_t *perm, const float *scale, int fmt, int loop,
                        int block, float *Wq, uint8_t *codes, void *ws, size_t ws_bytes);
int tg_pack_e8m0(void *stream, const uint8_t *e8m0, int m, int G, uint8_t *out);
int tg_dequant_mx(void *stream, const int32_t *qweight, const uint8_t *scales_e8m0, int fmt, int m,
                  int n, void *out, int out_dtype, int64_t stride_o);
int tg_qgemm_mx(void *stream, const void *X, int x_dtype, int T, int64_t stride_x,
                const int32_t *qweight, const uint8_t *scales_e8m0, int fmt, int m, int n,
                const void *bias, int bias_dtype, void *Y, int y_dtype, int64_t stride_y, void *ws,
                size_t ws_bytes);

/* ---- A16: MXFP8 activations (new; opt-in W4A8 for MXFP4 checkpoints) --------
 * `act_fmt` is a tg_act_format; TG_ACT_MXFP8 is its only value (anything else
 * is rejected with act_fmt's argument index).  Elements are e4m3fn in the OCP
 * encoding (bias 7, subnormals, largest finite 448 = 0x7e, no infinity; not
 * fnuz), one shared E8M0 byte per 32 values.  Every f32 operation below is one
 * correctly rounded operation in the order written.  Activations are finite;
 * NaN and Inf are outside the contract.
 *
 * Quantiser (tg_quant_act_mx; X is T x n of x_dtype TG_F16 / TG_BF16 with row
 * stride stride_x >= n, xq is T x n bytes with row stride stride_q >= n, xs is
 * T x n/32 bytes, contiguous).  Blocks: 32 consecutive columns of one row;
 * n % 32 == 0.
 *   a = max |x| over the block, converted exactly to f32;
 *   byte = max(exponent_field(a) - 8, 0), exponent_field the biased 8-bit field
 *     of a's f32 encoding and 8 e4m3's emax (a == 0 and f32 subnormals: byte 0);
 *     byte <= 246, so 255 (NaN) is never written;
 *   t = x * 2^(127 - byte): exact, but for results below the f32 normal range,
 *     which lie far below the smallest e4m3 tie 2^-10 and become zero either way;
 *   q = t rounded to nearest, ties to even, onto the e4m3fn grid, the subnormals
 *     (multiples of 2^-9 below 2^-6) included; |t| > 448 saturates to +-448
 *     (|t| < 512 by construction, so the rounding never reaches the NaN code).
 *   Sign: the sign bit of q is the sign bit of x, always: -0 and negative values
 *     that round to zero give 0x80, which decodes to -0 and multiplies as zero.
 * X may be a strided view; loads are 16 bytes wide where X and stride_x allow
 * it and scalar otherwise, the stores of xq likewise.
 *
 * tg_qgemm_mx_act: Y (T x m, row stride stride_y >= m) = X^ * W^^T (+ bias).
 * X^ is exactly tg_quant_act_mx's output decoded, float(e4m3(q)) * 2^(byte -
 * 127); W^ is exactly tg_dequant_mx's TG_F32 output of the packed pair.  Both
 * go to v_mfma_scale_f32_16x16x128_f8f6f4 as they lie in memory: no weight is
 * decoded outside the matrix pipe.  Accumulation is f32 (inside a 128-value
 * step in the instruction's own order, across steps in ascending k); the bias
 * (m, nullable, TG_F16 / TG_BF16 / TG_F32) is added in f32; one rounding to
 * y_dtype TG_F16 / TG_BF16 / TG_F32.  Bit-identical from call to call.
 * One regime for every T (no TG_QGEMM switch): the activations are quantised
 * once into the workspace, then a workgroup owns (16 rows up to T = 32, above
 * 64) x 64 features and walks K in steps of 128; while the output tiles
 * are fewer than ~512 workgroups K is split into S parts of at least 4 steps
 * and a second kernel adds the partial sums [S][T][m] in ascending order, then
 * the bias.  Requires n % 32 == 0 and (m * 4) % 32 == 0.
 * Weight scale bytes 0 .. 254 are accepted.  The instruction applies both
 * scales to the products exactly and produces f32 subnormals; a product below
 * 2^-149 becomes zero and one above the f32 range becomes inf (measured:
 * DESIGN.md "MXFP8 activations").
 * tg_qgemm_mx_act_workspace_size(T, m, n): X^ with T rounded up to 16 and n
 * to 128 (2048 + 64 bytes per 16 rows x 128 columns; the kernel keeps it in the
 * instruction's operand order), plus S*T*m*4 bytes when S > 1, plus alignment
 * slack; ws is never null. */
enum tg_act_format { TG_ACT_MXFP8 = 1 };
int tg_quant_act_mx(void *stream, const void *X, int x_dtype, int T, int64_t stride_x, int n,
                    int act_fmt, uint8_t *xq, int64_t stride_q, uint8_t *xs);
size_t tg_qgemm_mx_act_workspace_size(int T, int m, int n);
int tg_qgemm_mx_act(void *stream, const void *X, int x_dtype, int T, int64_t stride_x,
                    const int32_t *qweight, const uint8_t *scales_e8m0, int fmt, int act_fmt,
                    int m, int n, const void *bias, int bias_dtype, void *Y, int y_dtype,
                    int64_t stride_y, void *ws, size_t ws_bytes);

/* ---- A17: low-rank correction of the quantisation residual (new; absent in
 * the reference, which writes back dense FP16) -------------------------------
 * The best rank-r correction A B of E = W - Wq (m x n f32, row stride stride_e)
 * under the solver's objective, min tr((E - A B) H (E - A B)^T): A B = Q Q^T E
 * with Q the top-r eigenvectors of K = E H E^T (LoRC / LQER / QERA; DESIGN.md
 * "Low-rank correction").  H comes in one of two forms:
 *   gram = 0: a factor F (p x n, row stride stride_f, f_dtype TG_F64 or TG_F32,
 *             converted exactly to f64) with H = Fg^T Fg, Fg[:, perm[j]] =
 *             F[:, j]; perm (n int64, a permutation; null = identity) lets R_x
 *             be passed as process_hessian_alt returns it, and the scaled
 *             sketch Y goes in as it is (TG_F32, no perm).  M = E Fg^T (m x p);
 *             m <= p: K = M M^T, Q its eigenvectors; m > p: K = M^T M with
 *             eigenpairs (mu, P), Q = M P mu^-1/2.  The eigenproblem has order
 *             min(m, p).
 *   gram = 1: F is H itself (n x n f64, row stride stride_f; p is ignored,
 *             perm must be null); K = (E H) E^T, m x m.
 * 1 <= r <= 128 and r <= min(m, n).  Everything runs in FP64 on the library's
 * GEMM, SYRK and eigensolver (tg_eigh_values, tg_eigh_vectors_range; the call
 * synchronises the stream where they do).
 * Outputs: A0 = Q, B0 = Q^T E, balanced per direction by the power of two
 * s_j = 2^rint(log2(max|B0_j| / max|A0_j|) / 2): A[:, j] = A0_j s_j (m x r, row
 * stride stride_a), B[j, :] = B0_j / s_j (r x n, row stride stride_b), both of
 * ab_dtype TG_F32 (one rounding of the f64 value) or TG_F64 (what the tests
 * compare).  Directions with mu_j <= n 2^-52 mu_1, and directions past
 * min(m, p), come back as zero columns of A and zero rows of B, with mu_j = 0.
 * mu (r doubles, descending), err0 = tr K, and rank (int32, the number of kept
 * directions) are device memory; the weighted error after the correction is
 * err0 - sum(mu).  Deterministic. */
size_t tg_lrc_workspace_size(int m, int n, int p, int r, int gram);
int tg_lrc_factor(void *stream, const float *E, int m, int n, int64_t stride_e, const void *F,
                  int f_dtype, int p, int64_t stride_f, const int64_t *perm, int gram, int r,
                  void *A, int64_t stride_a, void *B, int64_t stride_b, int ab_dtype, double *mu,
                  double *err0, int32_t *rank, void *ws, size_t ws_bytes);

/* The correction at inference: Y = X W^^T + (X B^T) A^T + bias, beside the
 * packed GEMM and independent of its format.  The caller runs tg_qgemm /
 * tg_qgemm_mx / tg_qgemm_mx_act with y_dtype TG_F32 and no bias into Y32, then
 *   tg_lr_down:   Z (T x r f32, row stride stride_z) = X B^T, X (T x n, TG_F16 /
 *                 TG_BF16, row stride stride_x), B (r x n, TG_F16 / TG_BF16 /
 *                 TG_F32, row stride stride_b); 1 <= r <= 128, n % 8 == 0;
 *   tg_lr_finish: Y[t, o] = round(Y32[t, o] + sum_j Z[t, j] A[o, j] + bias[o]),
 *                 Y32 (T x m f32), A (m x r, TG_F16 / TG_BF16 / TG_F32), bias (m,
 *                 nullable, the same three types), Y (T x m, row stride stride_y
 *                 >= m) of y_dtype TG_F16 / TG_BF16 / TG_F32; Y may be Y32.
 * Numerics: X, B and A are converted exactly to f32 and every product and sum
 * is an f32 fma.  tg_lr_finish starts from Y32[t, o], adds the terms in
 * ascending j, then the bias, and rounds once.  tg_lr_down sums k in a fixed
 * order that depends on the regime and on (T, r, n) only; both calls are
 * bit-identical from call to call (no atomics).
 * tg_lr_down has two regimes (TG_LR_DOWN = auto | gemv | mfma, read per call;
 * gemv with T > 16 is an argument error, -4): gemv (T <= 16, the auto choice
 * there), one wave per row of B over a K chunk of a multiple of 512 values; mfma,
 * a 128 x 32 tile of Z per workgroup on v_mfma_f32_32x32x2_f32 with K slabs of
 * 32.  Both split K until about 512 workgroups run (gemv: chunks of at least
 * 512 values; mfma: at least 256); with S > 1 splits the partial sums [S][T][r]
 * go to the workspace and are added in ascending split order.  16-byte loads
 * are taken from X, B and A where the pointer and the row stride allow them
 * (16-bit: stride % 8 == 0; f32: stride % 4 == 0), scalar loads otherwise.
 * tg_lr_down_workspace_size(T, r, n): S*T*r*4 bytes (+ alignment slack) for the
 * larger S of the regimes that take T, 0 when that is 1. */
size_t tg_lr_down_workspace_size(int T, int r, int n);
int tg_lr_down(void *stream, const void *X, int x_dtype, int T, int64_t stride_x, const void *B,
               int b_dtype, int r, int n, int64_t stride_b, float *Z, int64_t stride_z, void *ws,
               size_t ws_bytes);
int tg_lr_finish(void *stream, const float *Y32, int64_t stride_y32, const float *Z,
                 int64_t stride_z, const void *A, int a_dtype, int64_t stride_a, int T, int m,
                 int r, const void *bias, int bias_dtype, void *Y, int y_dtype, int64_t stride_y);

/* ---- A18: randomised block-Hadamard rotation (new; the reference's roadmap
 * lists it as "integration with QuIP#") -----------------------------------------
 * Q = diag(s) (I_{n/b} (x) H_b) c, with b = block a power of two in [32, 4096]
 * that divides n, H_b the Sylvester Hadamard matrix, c = 1/sqrt(b) and s in
 * {+1, -1}^n.  x W^T = (x Q)(W Q)^T holds exactly, and the rotated W and H have
 * no outlier columns (DESIGN.md "Hadamard rotation").
 * sign_bits: n / 32 int32 words of device memory, bit j of word i set = column
 * 32 i + j is negated; null = all signs +.
 * The row operator R(x) = x Q, operation by operation (the host restatement is
 * bit-equal, tests/had_ref.py):
 *   1. x is converted exactly to the compute type, f64 for TG_F64 input and f32
 *      otherwise;
 *   2. every element is multiplied by its sign (exact);
 *   3. inside each block of b consecutive columns the stages h = 1, 2, 4, ...
 *      b/2 run in that order; stage h turns every pair (j, j + h) with
 *      (j mod 2h) < h into (u + v, u - v), each one correctly rounded operation;
 *   4. one multiply by c = (float)(1.0 / sqrt((double)b)), or its f64 form (a
 *      power of two when log2 b is even);
 *   5. one round-to-nearest-even to the output type.
 * The inverse R^-1(y) = y Q^T has the same steps 1, 3 and 4 and multiplies by
 * the signs after the scale.
 * tg_hadamard applies R (inverse = 0) or R^-1 to each of `rows` rows of X
 * (x_dtype TG_F16 / TG_BF16 / TG_F32 / TG_F64, row stride stride_x >= n) into Y
 * (y_dtype TG_F16 / TG_BF16 / TG_F32, or TG_F64 exactly when x_dtype is; row
 * stride stride_y >= n).  Y may be X when the dtypes and strides are equal.
 * 16-byte loads and stores are used where the pointer and the row stride in
 * bytes are multiples of 16, scalar ones otherwise.  One launch, one pass over
 * memory, bit-identical from call to call.
 * tg_hadamard_sym: H (n x n f64, row stride stride_h) <- Q^T H Q in place: the
 * row operator on every row, then the same operator along the row index; the
 * lower triangle, diagonal included, is what that gives and the upper triangle
 * is written as its mirror, so H is exactly symmetric.  No workspace. */
int tg_hadamard(void *stream, const void *X, int x_dtype, int64_t rows, int n, int64_t stride_x,
                int block, const int32_t *sign_bits, int inverse, void *Y, int y_dtype,
                int64_t stride_y);
int tg_hadamard_sym(void *stream, double *H, int n, int64_t stride_h, int block,
                    const int32_t *sign_bits);

#ifdef __cplusplus
}
#endif
#endif /* TRUNCGPTQ_H */
