// Blocked Householder QR, R only, FP64, for gfx950 (tg_qr_r and the fallback of
// the U factors in ufactor.hip; the reference's QR is gptq_utils.py:120).
//
// Communication-avoiding (TSQR-tree) form: no launch waits on another
// workgroup.  For each panel of HB = 32 columns starting at j0 (m = k - j0
// rows):
//   leaf    one workgroup per block of HR = 256 panel rows: the 256 x 32 slice
//           goes to LDS, up to 32 true Householder steps run there (scaled column
//           norm by workgroup reduction, beta = -sign(x0) |x|, v with unit head; a
//           zero column gives tau = 0), V and the 32 x 32 T of the compact-WY
//           form go to scratch, the block's R to its first 32 rows, zeros below;
//   tree    the first 32 rows of up to 8 neighbouring blocks form one 256-row
//           block (an index map, RowMap, not a copy) for the same kernel, until
//           one block remains: the panel's R then sits in rows j0 .. j0 + 31;
//   apply   after every factor launch, grid = blocks x 64-column tiles of the
//           trailing columns: C_blk -= V (T^T (V^T C_blk)) on the block's rows
//           through the same map, FP64 MFMA.
// Stream order puts a level's apply after its factor and before the next
// level's factor.  Every sum runs in a fixed order, so two calls on the same
// input agree bit for bit; loop bounds depend on (k, n) only.  A non-finite
// column norm, or a non-finite entry of the finished R, sets the device info
// word, which the host reads once at the end.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <type_traits>

#include "../../include/truncgptq.h"
#include "common.h"
#include "reduce.h"

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int HB = 32;    // panel width
constexpr int HR = 256;   // rows of one block
constexpr int HFAN = 8;   // blocks gathered per tree node (HFAN * HB = HR)
constexpr int HP = HB + 1;
constexpr int HTN = 64;   // trailing columns per apply workgroup (16 per wave)

// Local row r of block blk -> matrix row:
//   leaf (cs = 256, fan = 1, stride = 256): j0 + blk * 256 + r;
//   tree level L >= 1 (cs = 32, fan = 8, stride = 256 * 8^(L-1)): chunk r / 32
//   is the top of child block blk * 8 + r / 32 of the level below.
// Rows >= k do not exist; the existing rows of a block are a prefix of it.
struct RowMap {
  int j0, cs, fan;
  int64_t stride;
};

__device__ inline int64_t map_row(const RowMap &m, int blk, int r) {
  return int64_t(m.j0) + (int64_t(blk) * m.fan + r / m.cs) * m.stride + r % m.cs;
}

// Block-wide maximum of one non-negative double per thread (all threads get it).
__device__ inline double block_max(double v, double *scratch /* >= 4 doubles */) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < int(blockDim.x >> 6); ++w) s = fmax(s, scratch[w]);
  return s;
}

// One block of one panel: Householder QR of its (up to) 256 x b slice.
// Vb: rows blk * 256 + r (existing rows only) x 32; Tb: blk x 32 x 32.
__global__ __launch_bounds__(HR) void hqr_panel_kernel(double *__restrict__ A, int64_t lda, int k,
                                                      int b, RowMap m, double *__restrict__ Vb,
                                                      double *__restrict__ Tb,
                                                      int *__restrict__ info) {
  __shared__ double P[HR][HP];
  __shared__ double Gs[HB][HP];
  __shared__ double Ts[HB][HP];
  __shared__ double part[HR / HB][HB];
  __shared__ double vcol[HR];
  __shared__ double wv[HB];
  __shared__ double tau[HB];
  __shared__ double red[4], red2[4];
  const int t = threadIdx.x, blk = blockIdx.x;
  for (int idx = t; idx < HR * HB; idx += HR) {
    const int r = idx >> 5, c = idx & 31;
    const int64_t row = map_row(m, blk, r);
    P[r][c] = (row < k && c < b) ? A[row * lda + m.j0 + c] : 0.0;
  }
  __syncthreads();
  for (int j = 0; j < HB; ++j) {
    const double x = t >= j ? P[t][j] : 0.0;
    // scaled 2-norm (as dnrm2): no overflow / underflow of the squares.  fmax
    // drops a NaN, the sum does not: a NaN entry still gives nx = NaN, and an
    // Inf scale gives Inf / Inf = NaN.
    const double amax = block_max(fabs(x), red2);
    const double sc = amax > 0.0 ? amax : 1.0;
    const double y = x / sc;
    const double nx = sc * sqrt(tg::block_sum(y * y, red));
    const double x0 = P[j][j];
    double tj = 0.0, v = t == j ? 1.0 : 0.0, beta = x0;
    if (!(nx <= DBL_MAX)) {
      if (t == 0) *info = 1;  // non-finite input: every workgroup that sees it stores the same 1
    } else if (nx > 0.0) {
      beta = -copysign(nx, x0);
      tj = (beta - x0) / beta;
      if (t > j) v = x / (x0 - beta);
    }
    vcol[t] = v;
    __syncthreads();
    {  // w = tau v^T P[:, j+1:], 8 partial sums per column added in a fixed order
      const int c = t & 31, q = t >> 5;
      double s = 0.0;
      for (int r = q * HB; r < (q + 1) * HB; ++r) s += vcol[r] * P[r][c];
      part[q][c] = s;
    }
    __syncthreads();
    if (t < HB) {
      double s = 0.0;
      for (int q = 0; q < HR / HB; ++q) s += part[q][t];
      wv[t] = tj * s;
    }
    __syncthreads();
    if (tj != 0.0 && t >= j)
      for (int c = j + 1; c < HB; ++c) P[t][c] -= v * wv[c];
    if (t == j) P[t][j] = beta;
    if (t > j) P[t][j] = v;  // V below the diagonal, R on and above it
    if (t == 0) tau[j] = tj;
    __syncthreads();
  }
  // G = strict upper triangle of V^T V (V unit lower trapezoidal)
  for (int e = t; e < HB * HB; e += HR) {
    const int i = e >> 5, j = e & 31;
    double s = 0.0;
    if (i < j) {
      s = P[j][i];
      for (int r = j + 1; r < HR; ++r) s += P[r][i] * P[r][j];
    }
    Gs[i][j] = s;
  }
  __syncthreads();
  // T[:j, j] = -tau_j T[:j, :j] (V[:, :j]^T V[:, j]); row i of T belongs to thread i
  if (t < HB) {
    const int i = t;
    for (int j = 0; j < HB; ++j) {
      double val = 0.0;
      if (i == j) val = tau[j];
      if (i < j) {
        double s = 0.0;
        for (int l = i; l < j; ++l) s += Ts[i][l] * Gs[l][j];
        val = -tau[j] * s;
      }
      Ts[i][j] = val;
    }
  }
  __syncthreads();
  for (int idx = t; idx < HR * HB; idx += HR) {
    const int r = idx >> 5, c = idx & 31;
    const int64_t row = map_row(m, blk, r);
    if (row >= k) continue;
    Vb[(size_t(blk) * HR + r) * HB + c] = r < c ? 0.0 : r == c ? 1.0 : P[r][c];
    if (c < b) A[row * lda + m.j0 + c] = (r < HB && c >= r) ? P[r][c] : 0.0;
  }
  for (int idx = t; idx < HB * HB; idx += HR) Tb[size_t(blk) * HB * HB + idx] = Ts[idx >> 5][idx & 31];
}

// C_blk -= V (T^T (V^T C_blk)) for the block's rows and 64 trailing columns
// from c0 + blockIdx.y * 64; each wave owns 16 of them.
__global__ __launch_bounds__(256) void hqr_apply_kernel(double *__restrict__ A, int64_t lda, int k,
                                                        int n, int c0, RowMap m,
                                                        const double *__restrict__ Vb,
                                                        const double *__restrict__ Tb) {
  __shared__ double Ts[HB][HP];
  __shared__ double Ws[4][HB][17];
  __shared__ double W2[4][HB][17];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, blk = blockIdx.x;
  const int lr = lane >> 4, lc = lane & 15;
  for (int idx = t; idx < HB * HB; idx += 256) Ts[idx >> 5][idx & 31] = Tb[size_t(blk) * HB * HB + idx];
  const int64_t col = int64_t(c0) + int64_t(blockIdx.y) * HTN + w * 16 + lc;
  const bool colok = col < n;
  const double *V = Vb + size_t(blk) * HR * HB;
  // W = V^T C  (32 x 16 per wave)
  v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  for (int kk = 0; kk < HR; kk += 4) {
    const int r = kk + lr;
    const int64_t row = map_row(m, blk, r);
    const bool rok = row < k;
    const double bv = (rok && colok) ? A[row * lda + col] : 0.0;
    const double a0 = rok ? V[size_t(r) * HB + lc] : 0.0;
    const double a1 = rok ? V[size_t(r) * HB + 16 + lc] : 0.0;
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bv, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bv, acc1, 0, 0, 0);
  }
  for (int r = 0; r < 4; ++r) {
    Ws[w][lr + 4 * r][lc] = acc0[r];
    Ws[w][16 + lr + 4 * r][lc] = acc1[r];
  }
  __syncthreads();
  // W2 = T^T W  (T upper triangular)
  for (int e = lane; e < HB * 16; e += 64) {
    const int i = e >> 4, j = e & 15;
    double s = 0.0;
    for (int l = 0; l <= i; ++l) s += Ts[l][i] * Ws[w][l][j];
    W2[w][i][j] = s;
  }
  __syncthreads();
  double bf[HB / 4];
  for (int q = 0; q < HB / 4; ++q) bf[q] = W2[w][4 * q + lr][lc];
  // C -= V W2
  for (int rt = 0; rt < HR / 16; ++rt) {
    const int ra = rt * 16 + lc;
    const bool aok = map_row(m, blk, ra) < k;
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < HB / 4; ++q) {
      const double a = aok ? V[size_t(ra) * HB + 4 * q + lr] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bf[q], acc, 0, 0, 0);
    }
    for (int r = 0; r < 4; ++r) {
      const int64_t row = map_row(m, blk, rt * 16 + lr + 4 * r);
      if (row < k && colok) A[row * lda + col] -= acc[r];
    }
  }
}

// Rows with a negative diagonal entry are negated (columns i .. n-1), and the
// whole upper trapezoid is checked for non-finite entries (a NaN / Inf in a
// trailing input column never meets a column norm, but it stays in R).
// Every thread reads the diagonal entry before the barrier; stores follow it.
__global__ __launch_bounds__(256) void hqr_sign_kernel(double *__restrict__ A, int64_t lda, int k,
                                                       int n, int *__restrict__ info) {
  const int i = blockIdx.x;
  double *row = A + int64_t(i) * lda;
  const bool neg = row[i] < 0.0;
  __syncthreads();
  bool bad = false;
  for (int j = i + threadIdx.x; j < n; j += 256) {
    const double v = row[j];
    bad |= !(fabs(v) <= DBL_MAX);
    if (neg) row[j] = -v;
  }
  if (bad) *info = 1;
}

struct HqrWs {
  double *V, *T;
  int *info;
};

template <class Ar>
void hqr_layout(Ar &ar, int k, HqrWs *w) {
  HqrWs d{};
  HqrWs &q = w ? *w : d;
  const size_t nb = size_t(tg::cdiv(k, HR));
  auto t = [&](auto *&dst, size_t cnt) {
    using T = std::remove_reference_t<decltype(*dst)>;
    dst = ar.template take<T>(cnt);
  };
  t(q.V, size_t(k) * HB);
  t(q.T, nb * HB * HB);
  t(q.info, 16);
}

}  // namespace

namespace tg {

size_t hqr_scratch_bytes(int k) {
  Sizer s;
  hqr_layout(s, k, nullptr);
  return s.off;
}

// In-place R of the k x n row-major A (ld lda >= n, 1 <= k <= n); scratch of
// hqr_scratch_bytes(k) bytes, 256-byte aligned.  Synchronises the stream once.
int hqr_r(hipStream_t st, double *A, int64_t lda, int k, int n, void *scratch, size_t bytes) {
  Arena ar(scratch, bytes);
  HqrWs w{};
  hqr_layout(ar, k, &w);
  if (!ar.ok()) {
    set_error("Householder QR: scratch too small (%zu > %zu bytes)", ar.off, ar.cap);
    return -99;
  }
  TG_HIP(hipMemsetAsync(w.info, 0, sizeof(int), st));
  for (int j0 = 0; j0 < k; j0 += HB) {
    const int b = std::min(HB, k - j0), c0 = j0 + b;
    int nb = cdiv(k - j0, HR);
    RowMap m{j0, HR, 1, HR};
    for (;;) {
      hipLaunchKernelGGL(hqr_panel_kernel, dim3(nb), dim3(HR), 0, st, A, lda, k, b, m, w.V, w.T,
                         w.info);
      TG_LAUNCHED();
      if (n > c0) {
        hipLaunchKernelGGL(hqr_apply_kernel, dim3(nb, cdiv(n - c0, HTN)), dim3(256), 0, st, A, lda,
                           k, n, c0, m, w.V, w.T);
        TG_LAUNCHED();
      }
      if (nb == 1) break;
      m = RowMap{j0, HB, HFAN, m.cs == HR ? int64_t(HR) : m.stride * HFAN};
      nb = cdiv(nb, HFAN);
    }
  }
  hipLaunchKernelGGL(hqr_sign_kernel, dim3(k), dim3(256), 0, st, A, lda, k, n, w.info);
  TG_LAUNCHED();
  int h_info = 0;
  TG_HIP(hipMemcpyAsync(&h_info, w.info, sizeof(int), hipMemcpyDeviceToHost, st));
  TG_HIP(hipStreamSynchronize(st));
  if (h_info != 0) {
    set_error("Householder QR broke down (non-finite input)");
    return int(hipErrorUnknown);
  }
  return 0;
}

}  // namespace tg

extern "C" size_t tg_qr_r_workspace_size(int k, int n) {
  (void)n;
  if (k < 1) return 256;
  return tg::hqr_scratch_bytes(k) + 256;
}

extern "C" int tg_qr_r(void *stream, double *A, int lda, int k, int n, void *ws, size_t ws_bytes) {
  TG_ARG(A, 2, "null A");
  TG_ARG(n >= 1, 5, "n < 1");
  TG_ARG(lda >= n, 3, "lda < n");
  TG_ARG(k >= 1 && k <= n, 4, "k must be in [1, n]");
  TG_ARG(ws, 6, "null ws");
  tg::Arena ar(ws, ws_bytes);
  char *base = ar.take_aligned<char>(tg::hqr_scratch_bytes(k), 256);
  TG_WS(ar);
  return tg::hqr_r((hipStream_t)stream, A, lda, k, n, base, tg::hqr_scratch_bytes(k));
}
