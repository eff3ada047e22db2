// A17: low-rank correction of a quantisation residual under the solver's own
// objective (no reference counterpart: the reference writes back dense FP16).
//
//   min over rank-r A B of  tr((E - A B) H (E - A B)^T),   E = W - Wq (m x n)
//
// With H = F^T F the objective is ||(E - A B) F^T||_F^2, so by Eckart-Young the
// minimiser is A B = Q Q^T E with Q (m x r) the top-r left singular vectors of
// M = E F^T, i.e. the top-r eigenvectors of K = M M^T = E H E^T; the weighted
// error falls from err0 = tr K to err0 - (mu_1 + .. + mu_r), mu the top
// eigenvalues of K.  Everything below is FP64 on the library's own GEMM / SYRK
// (gemm64.hip) and eigensolver (eigh.hip); this file adds only the streaming
// pieces around them: the conversion of E, the gather of F through perm, the
// symmetrisation and the trace of K, the choice of the kept directions, the
// mu^-1/2 scaling and the power-of-two balancing that writes A and B.
//
// Routes (the eigenproblem has order q = min(m, p), or m with gram = 1):
//   gram = 1      K = (E H) E^T (m x m), Q = its top eigenvectors;
//   gram = 0, m <= p   M = E F^T (m x p), K = M M^T (m x m), Q likewise;
//   gram = 0, m > p    K = M^T M (p x p) with eigenpairs (mu, P),
//                      Q = M P mu^-1/2.
#include <algorithm>

#include "../../include/truncgptq.h"
#include "common.h"
#include "gemm64.h"
#include "reduce.h"

namespace {

// dst (rows x cols f64, ld cols) = double(src (rows x cols, row stride lds))
template <class T>
__global__ void lrc_to_f64_kernel(const T *__restrict__ src, int64_t lds, int rows, int cols,
                                  double *__restrict__ dst) {
  for (int64_t r = blockIdx.y; r < rows; r += gridDim.y)
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < cols; c += gridDim.x * blockDim.x)
      dst[r * cols + c] = double(src[r * lds + c]);
}

// Fg[:, perm[j]] = F[:, j] (perm a permutation of 0 .. n-1; null = identity),
// so that H = Fg^T Fg is in E's column order
template <class T>
__global__ void lrc_gather_kernel(const T *__restrict__ F, int64_t ldf, int p, int n,
                                  const int64_t *__restrict__ perm, double *__restrict__ Fg) {
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) {
    const int64_t d = perm ? perm[c] : int64_t(c);
    for (int64_t r = blockIdx.y; r < p; r += gridDim.y) Fg[r * n + d] = double(F[r * ldf + c]);
  }
}

// K <- (K + K^T) / 2: thread (i, j), i > j, owns the pair
__global__ void lrc_symmetrise_kernel(double *__restrict__ K, int q) {
  for (int i = blockIdx.y; i < q; i += gridDim.y)
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < i; j += gridDim.x * blockDim.x) {
      const double v = 0.5 * (K[size_t(i) * q + j] + K[size_t(j) * q + i]);
      K[size_t(i) * q + j] = v;
      K[size_t(j) * q + i] = v;
    }
}

// err0 = tr K, summed in a fixed order (one workgroup)
__global__ __launch_bounds__(256) void lrc_trace_kernel(const double *__restrict__ K, int q,
                                                        double *__restrict__ err0) {
  __shared__ double red[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < q; i += 256) s += K[size_t(i) * q + i];
  s = tg::block_sum(s, red);
  if (threadIdx.x == 0) *err0 = s;
}

// The kept directions: mu_j > n 2^-52 mu_1 (a prefix, the spectrum descends).
// mu[j] = the eigenvalue, or 0 for a dropped direction; sc[j] = the factor that
// turns row j of the eigenvector product into a unit vector (1 on the m-route,
// mu^-1/2 on the p-route), or 0 for a dropped direction.
__global__ __launch_bounds__(128) void lrc_select_kernel(const double *__restrict__ w_asc, int q,
                                                         int re, int r, int n, int proute,
                                                         double *__restrict__ mu,
                                                         double *__restrict__ sc,
                                                         int32_t *__restrict__ rank) {
  const int j = threadIdx.x;
  const double mu1 = w_asc[q - 1];
  const double thr = double(n) * 0x1p-52 * mu1;
  const double v = j < re ? w_asc[q - 1 - j] : 0.0;
  const bool keep = j < re && mu1 > 0.0 && v > thr;
  const int kept = __syncthreads_count(keep);
  if (j < r) {
    mu[j] = keep ? v : 0.0;
    sc[j] = keep ? (proute ? 1.0 / sqrt(v) : 1.0) : 0.0;
  }
  if (j == 0) *rank = kept;
}

// Qt[j, :] = sc[j] * src[j, :] (rows j < re; a dropped row becomes exactly 0
// whatever src holds).  src may be Qt itself.
__global__ void lrc_scale_rows_kernel(const double *src, int64_t lds, int cols,
                                      const double *__restrict__ sc, double *Qt) {
  const int j = blockIdx.y;
  const double s = sc[j];
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < cols; c += gridDim.x * blockDim.x)
    Qt[size_t(j) * cols + c] = s != 0.0 ? s * src[size_t(j) * lds + c] : 0.0;
}

__device__ inline double block_max(double v, double *scratch) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < int(blockDim.x >> 6); ++w) s = fmax(s, scratch[w]);
  return s;
}

// One workgroup per direction j: s = 2^rint(log2(max|B0_j| / max|A0_j|) / 2),
// A[:, j] = A0_j s, B[j, :] = B0_j / s (exact scalings, so A B is unchanged bit
// for bit); a dropped direction (sc[j] == 0) or an all-zero row gives zeros.
template <class T>
__global__ __launch_bounds__(256) void lrc_balance_kernel(const double *__restrict__ Qt, int m,
                                                          const double *__restrict__ B0, int n,
                                                          const double *__restrict__ sc,
                                                          T *__restrict__ A, int64_t lda,
                                                          T *__restrict__ B, int64_t ldb) {
  __shared__ double red[4];
  const int j = blockIdx.x;
  const bool kept = sc[j] != 0.0;  // uniform over the workgroup
  double ma = 0.0, mb = 0.0;
  if (kept) {
    for (int i = threadIdx.x; i < m; i += 256) ma = fmax(ma, fabs(Qt[size_t(j) * m + i]));
    for (int c = threadIdx.x; c < n; c += 256) mb = fmax(mb, fabs(B0[size_t(j) * n + c]));
  }
  ma = block_max(ma, red);
  mb = block_max(mb, red);
  const bool live = kept && ma > 0.0 && mb > 0.0 && isfinite(ma) && isfinite(mb);
  if (!live) {  // rows j >= min(r, q) of Qt and B0 do not exist: nothing is read here
    for (int i = threadIdx.x; i < m; i += 256) A[size_t(i) * lda + j] = T(0);
    for (int c = threadIdx.x; c < n; c += 256) B[size_t(j) * ldb + c] = T(0);
    return;
  }
  const int e = int(fmin(fmax(rint(0.5 * log2(mb / ma)), -1000.0), 1000.0));
  const double up = ldexp(1.0, e), down = ldexp(1.0, -e);
  for (int i = threadIdx.x; i < m; i += 256)
    A[size_t(i) * lda + j] = T(Qt[size_t(j) * m + i] * up);
  for (int c = threadIdx.x; c < n; c += 256)
    B[size_t(j) * ldb + c] = T(B0[size_t(j) * n + c] * down);
}

struct LrcBufs {
  double *E64, *F64, *M, *K, *w, *Vh, *Qt, *B0, *sc;
  void *eigh;
  size_t eigh_bytes;
};

int lrc_order(int m, int p, int gram) { return gram ? m : std::min(m, p); }

template <class A>
void lrc_layout(A &ar, int m, int n, int p, int r, int gram, LrcBufs *b) {
  const int q = lrc_order(m, p, gram);
  const int re = std::min(r, q);
  const size_t counts[9] = {size_t(m) * n,                      // E64
                            gram ? size_t(m) * n : size_t(p) * n,  // E H, or the gathered F
                            gram ? 0 : size_t(m) * p,           // M
                            size_t(q) * q,                      // K
                            size_t(q),                          // w_asc
                            size_t(re) * q,                     // Vh
                            size_t(re) * m,                     // Qt
                            size_t(re) * n,                     // B0
                            size_t(r)};                         // sc
  double *ptrs[9] = {};
  for (int i = 0; i < 9; ++i) ptrs[i] = ar.template take<double>(counts[i]);
  const size_t eb = tg_eigh_workspace_size(q);
  char *ep = ar.template take<char>(eb);
  if (b) *b = LrcBufs{ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6], ptrs[7],
                      ptrs[8], ep, eb};
}

// rows on y (the kernels stride over y: the grid's y extent ends at 65535)
dim3 row_grid(int cols, int rows) {
  return dim3(std::min(64, tg::cdiv(cols, 256)), std::min(rows, 65535));
}

}  // namespace

extern "C" size_t tg_lrc_workspace_size(int m, int n, int p, int r, int gram) {
  if (m < 1 || n < 1 || r < 1 || (!gram && p < 1)) return 0;
  tg::Sizer s;
  lrc_layout(s, m, n, gram ? n : p, r, gram ? 1 : 0, nullptr);
  return s.off + 256;
}

extern "C" int tg_lrc_factor(void *stream, const float *E, int m, int n, int64_t stride_e,
                             const void *F, int f_dtype, int p, int64_t stride_f,
                             const int64_t *perm, int gram, int r, void *A, int64_t stride_a,
                             void *B, int64_t stride_b, int ab_dtype, double *mu, double *err0,
                             int32_t *rank, void *ws, size_t ws_bytes) {
  TG_ARG(E, 2, "null E");
  TG_ARG(m >= 1, 3, "m < 1");
  TG_ARG(n >= 1, 4, "n < 1");
  TG_ARG(stride_e >= n, 5, "stride_e < n");
  TG_ARG(F, 6, "null F / H");
  TG_ARG(gram == 0 || gram == 1, 11, "gram must be 0 or 1");
  TG_ARG(f_dtype == TG_F64 || (!gram && f_dtype == TG_F32), 7,
         "F must be f64 or f32, H must be f64");
  if (gram) p = n;
  TG_ARG(p >= 1, 8, "p < 1");
  TG_ARG(stride_f >= n, 9, "stride_f < n");
  TG_ARG(!(gram && perm), 10, "perm goes with a factor, not with H");
  TG_ARG(r >= 1 && r <= 128 && r <= std::min(m, n), 12, "r must be in [1, min(128, m, n)]");
  TG_ARG(A, 13, "null A");
  TG_ARG(stride_a >= r, 14, "stride_a < r");
  TG_ARG(B, 15, "null B");
  TG_ARG(stride_b >= n, 16, "stride_b < n");
  TG_ARG(ab_dtype == TG_F32 || ab_dtype == TG_F64, 17, "A / B must be f32 or f64");
  TG_ARG(mu, 18, "null mu");
  TG_ARG(err0, 19, "null err0");
  TG_ARG(rank, 20, "null rank");
  hipStream_t st = static_cast<hipStream_t>(stream);
  tg::Arena ar(ws, ws_bytes);
  LrcBufs b{};
  lrc_layout(ar, m, n, p, r, gram, &b);
  TG_WS(ar);
  const int q = lrc_order(m, p, gram);
  const int re = std::min(r, q);
  const bool proute = !gram && m > p;

  hipLaunchKernelGGL(lrc_to_f64_kernel<float>, row_grid(n, m), dim3(256), 0, st, E, stride_e, m,
                     n, b.E64);
  TG_LAUNCHED();
  const double *M = nullptr;
  if (gram) {
    const double *H = static_cast<const double *>(F);
    TG_HIP(tg::dgemm(st, false, false, m, n, n, 1.0, b.E64, n, H, stride_f, 0.0, b.F64, n));
    TG_HIP(tg::dgemm(st, false, true, m, m, n, 1.0, b.F64, n, b.E64, n, 0.0, b.K, m));
    if (m > 1) {
      hipLaunchKernelGGL(lrc_symmetrise_kernel, row_grid(m, m), dim3(256), 0, st, b.K, m);
      TG_LAUNCHED();
    }
  } else {
    if (f_dtype == TG_F64)
      hipLaunchKernelGGL(lrc_gather_kernel<double>, row_grid(n, p), dim3(256), 0, st,
                         static_cast<const double *>(F), stride_f, p, n, perm, b.F64);
    else
      hipLaunchKernelGGL(lrc_gather_kernel<float>, row_grid(n, p), dim3(256), 0, st,
                         static_cast<const float *>(F), stride_f, p, n, perm, b.F64);
    TG_LAUNCHED();
    TG_HIP(tg::dgemm(st, false, true, m, p, n, 1.0, b.E64, n, b.F64, n, 0.0, b.M, p));
    M = b.M;
    if (proute)
      TG_HIP(tg::dsyrk_tn(st, p, m, 1.0, M, p, 0.0, b.K, p));
    else
      TG_HIP(tg::dsyrk_nt(st, m, p, 1.0, M, p, 0.0, b.K, m));
  }
  hipLaunchKernelGGL(lrc_trace_kernel, dim3(1), dim3(256), 0, st, b.K, q, err0);
  TG_LAUNCHED();

  int rc = tg_eigh_values(st, b.K, q, q, b.w, b.eigh, b.eigh_bytes);
  if (rc) return rc;
  rc = tg_eigh_vectors_range(st, q, b.w, 0, re, b.Vh, q, b.eigh, b.eigh_bytes);
  if (rc) return rc;
  hipLaunchKernelGGL(lrc_select_kernel, dim3(1), dim3(128), 0, st, b.w, q, re, r, n,
                     proute ? 1 : 0, mu, b.sc, rank);
  TG_LAUNCHED();
  if (proute)  // Qt = mu^-1/2 P^T M^T
    TG_HIP(tg::dgemm(st, false, true, re, m, p, 1.0, b.Vh, q, M, p, 0.0, b.Qt, m));
  hipLaunchKernelGGL(lrc_scale_rows_kernel, row_grid(m, re), dim3(256), 0, st,
                     proute ? b.Qt : b.Vh, int64_t(m), m, b.sc, b.Qt);
  TG_LAUNCHED();
  TG_HIP(tg::dgemm(st, false, false, re, n, m, 1.0, b.Qt, m, b.E64, n, 0.0, b.B0, n));
  // directions re .. r-1 (only when r > q) have sc == 0 and are never read
  if (ab_dtype == TG_F32)
    hipLaunchKernelGGL(lrc_balance_kernel<float>, dim3(r), dim3(256), 0, st, b.Qt, m, b.B0, n,
                       b.sc, static_cast<float *>(A), stride_a, static_cast<float *>(B), stride_b);
  else
    hipLaunchKernelGGL(lrc_balance_kernel<double>, dim3(r), dim3(256), 0, st, b.Qt, m, b.B0, n,
                       b.sc, static_cast<double *>(A), stride_a, static_cast<double *>(B),
                       stride_b);
  TG_LAUNCHED();
  return 0;
}
