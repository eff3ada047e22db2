// U of the truncated spectral factorisation (A5) and the GPTQ comparator's
// factor: tg_u_factor, tg_u_factor_rx, tg_urx_*, tg_hinv_chol, with the
// blocked Cholesky, triangular-inverse and refinement machinery they share.
// The pivot order and R_x (A4) are in pivot.hip.
//
// Replaces, in the reference's gptq_utils.py:
//   torch.linalg.qr(H_inv_partial[:, perm]) + sign normalisation        :118-124
//       (cuSOLVER geqrf)                           -> tg_u_factor
//
// U.  U (k x n, upper trapezoidal, positive diagonal) is the R factor of
// A = diag(1/S_k) Vh_k[:, perm].  U^T U = A^T A, so U is the first k rows of
// the upper Cholesky factor of G = A^T A: form G[:k, :] = A[:, :k]^T A on
// FP64 MFMA, then a right-looking blocked Cholesky over those k rows (panel
// factor in LDS, triangular solve across all n columns, MFMA trailing update).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "../../include/truncgptq.h"
#include "common.h"
#include "gemm64.h"

namespace {

constexpr int CB = 32;    // Cholesky row panel for U

typedef double doublex4 __attribute__((ext_vector_type(4)));

// A[t][j] = (1/S[t]) * Vh[t][perm[j]]     (gptq_utils.py:111, 118-119)
__global__ void gather_scale_kernel(const double *__restrict__ Vh, int ldv, const double *__restrict__ S,
                                    const int64_t *__restrict__ perm, int n, double *__restrict__ A) {
  const int t = blockIdx.y;
  const double sinv = 1.0 / S[t];
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
    A[size_t(t) * n + j] = sinv * Vh[size_t(t) * ldv + perm[j]];
}

// Upper Cholesky of the pb x pb diagonal block at U[p][p] (in place), LDS.
// Diagonal block of the U Cholesky (NU x NU, in LDS): U11 = chol_upper(G11)
// written to U, and W = U11^-T (lower) to Wout, so the panel's off-diagonal
// rows become one MFMA GEMM U12 = W G12.  X = U11^-1 by back substitution,
// one column per thread group.
constexpr int NU = 64;
// Diagonal NU x NU block of the U Cholesky: U11 = chol_upper(G11) written to
// U and W = U11^-T (lower) to Wout, so the panel's off-diagonal rows become
// one MFMA GEMM U12 = W G12.  Four waves: lane c = column c, wave
// g holds rows 16g .. 16g + 15 (a[q] = A[16g + q][c]), so each wave issues a
// quarter of the update (a one-wave form, measured and removed, issued ≈17k
// instructions per block: 50 us against 31).  Step j: the owner wave publishes row j (columns < j as 0,
// so the update needs no mask: rows above j take multiplier 0, finished
// columns factor 0), one barrier, every wave updates its rows.  The inverse
// runs right-looking over U's columns: step l (descending) finalises row l of
// X = U^-1 in its owner, publishes it, and every wave subtracts
// U[i][l] X[l][:] from its rows i < l (U's diagonal held apart as 1/U_ll, so
// the stored column has zeros at i >= l).  Broadcast rows double-buffered:
// one barrier per step.
struct PotrfSm {
  double rowb[2][NU];
  double ut[NU][NU + 2];  // ut[l][i] = U[i][l] for i < l (0 elsewhere); then W = U11^-T
  double rinv[NU];
};
// The factor and the inverse of one diagonal block by the four waves of the
// calling workgroup (the steps described above): U11 ends in a[] (row RW g +
// q, column c, upper), W = U11^-T in sm.ut (ut[r][c] = W[r][c], lower), and
// the return value says a pivot of the block's pb rows was not positive.
// INV = false: the factor only (sm.ut then holds U's strict upper part).
// (Two pivots per barrier -- every thread forming the second pivot's row
// from the first's with the owner's fma, bit-identical -- measured no
// faster: the pivots' rsq / Newton chain, not the barriers, sets the pace.)
template <int NWV, bool INV>
__device__ __forceinline__ bool potrf_inv_block(const double *__restrict__ base, int ldu, int pb,
                                                PotrfSm &sm, double (&a)[NU / NWV]) {
  constexpr int RW = NU / NWV;  // rows per wave
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  {
    const int cc = min(c, pb - 1);
#pragma unroll
    for (int q = 0; q < RW; ++q) {
      const int r = RW * g + q;
      const double v = base[size_t(min(r, pb - 1)) * ldu + cc];  // clamped: no guarded loads
      a[q] = (r < pb && c < pb) ? v : (r == c ? 1.0 : 0.0);
    }
  }
  bool bad = false;
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    const int gj = j / RW, qj = j % RW;
    if (g == gj) sm.rowb[j & 1][c] = c >= j ? a[qj] : 0.0;
    __syncthreads();
    const double d = sm.rowb[j & 1][j];
    const double vc = sm.rowb[j & 1][c];
    double rv[RW];
    const double2 *r2 = reinterpret_cast<const double2 *>(&sm.rowb[j & 1][RW * g]);
#pragma unroll
    for (int q = 0; q < RW / 2; ++q) {
      const double2 t = r2[q];
      rv[2 * q] = t.x;
      rv[2 * q + 1] = t.y;
    }
    // 1/sqrt(d) by v_rsq_f64 + two Newton steps (the IEEE sqrt and division
    // are ~30 dependent instructions on the chain)
    double inv = __builtin_amdgcn_rsq(d);
    const double hd = 0.5 * d;
    inv = inv * fma(-hd * inv, inv, 1.5);
    inv = inv * fma(-hd * inv, inv, 1.5);
    const double piv = d * inv;
    bad |= !(d > 0.0) && j < pb;
    const double ujc = vc * inv;  // U[j][c] for c > j, 0 for c < j
    const double f = ujc * inv;
#pragma unroll
    for (int q = 0; q < RW; ++q) a[q] = fma(-rv[q], f, a[q]);  // rows <= j: rv = 0 or reset below
    if (g == gj) {
      a[qj] = c > j ? ujc : (c == j ? piv : 0.0);
      sm.ut[c][j] = c > j ? ujc : 0.0;  // column c of U at row j (diagonal apart)
    }
    if (c == j && g == 0) sm.rinv[j] = inv;
  }
  if constexpr (INV) {
    // X = U^-1: s = I, then for l = 63 .. 0: X[l] = s[l] / U_ll (owner), s[i] -= U[i][l] X[l]
    double x[RW];
#pragma unroll
    for (int q = 0; q < RW; ++q) x[q] = (RW * g + q == c) ? 1.0 : 0.0;
    __syncthreads();
#pragma unroll
    for (int l = NU - 1; l >= 0; --l) {
      const int gl = l / RW, ql = l % RW;
      if (g == gl) {
        x[ql] *= sm.rinv[l];
        sm.rowb[l & 1][c] = x[ql];
      }
      __syncthreads();
      const double xl = sm.rowb[l & 1][c];
      double uv[RW];
      const double2 *u2 = reinterpret_cast<const double2 *>(&sm.ut[l][RW * g]);
#pragma unroll
      for (int q = 0; q < RW / 2; ++q) {
        const double2 t = u2[q];
        uv[2 * q] = t.x;
        uv[2 * q + 1] = t.y;
      }
#pragma unroll
      for (int q = 0; q < RW; ++q) x[q] = fma(-uv[q], xl, x[q]);  // U[i][l] = 0 for i >= l
    }
    __syncthreads();  // ut is reused as the W buffer
    // W = X^T (lower): ut[c][r] = X[r][c]
#pragma unroll
    for (int q = 0; q < RW; ++q) {
      const int r = RW * g + q;
      sm.ut[c][r] = (r < pb && c < pb) ? x[q] : 0.0;
    }
    __syncthreads();
  }
  return bad;
}

template <int NWV>
__global__ __launch_bounds__(64 * NWV) void potrf_inv_4w_kernel(double *__restrict__ U, int ldu,
                                                                int p, int pb,
                                                                double *__restrict__ Wout,
                                                                int *__restrict__ info) {
  constexpr int RW = NU / NWV;
  __shared__ PotrfSm sm;
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  double a[RW];
  double *base = U + size_t(p) * ldu + p;
  const bool bad = potrf_inv_block<NWV, true>(base, ldu, pb, sm, a);
  if (threadIdx.x == 0 && bad) atomicAdd(info, 1);
  // U block (upper) back in place
#pragma unroll
  for (int q = 0; q < RW; ++q) {
    const int r = RW * g + q;
    if (r < pb && c < pb) base[size_t(r) * ldu + c] = c >= r ? a[q] : 0.0;
  }
#pragma unroll
  for (int q = 0; q < RW; ++q) {
    const int r = RW * g + q;
    Wout[r * NU + c] = sm.ut[r][c];
  }
}

// X = U11^-1 (64 x 64 upper) from potrf_inv_block<.., false>'s factor (U's
// strict upper part in sm.ut[l][i] = U[i][l], 1 / U_ll in sm.rinv) by
// blocks instead of 64 dependent row steps: the eight 8 x 8 diagonal blocks
// by back substitution (one thread per column, all at once), then three
// levels of X12 = -X11 (U12 X22) over blocks of 16, 32, 64 -- 7 barriers.
// xs: X (lower part zero); tmp: U12 X22 of the level.
__device__ __forceinline__ void trinv64_blocked(PotrfSm &sm, double (*xs)[NU + 1],
                                                double (*tmp)[NU + 1]) {
  const int tid = threadIdx.x;
  auto U = [&](int r, int c) { return r < c ? sm.ut[c][r] : 0.0; };  // strict upper
  for (int e = tid; e < NU * NU; e += 256) xs[e >> 6][e & 63] = 0.0;
  __syncthreads();
  if (tid < NU) {
    const int bb = 8 * (tid >> 3), c = tid & 7;
    double x[8];
#pragma unroll
    for (int i = 7; i >= 0; --i) {
      double acc = (i == c) ? 1.0 : 0.0;
#pragma unroll
      for (int kk = i + 1; kk < 8; ++kk) acc = fma(-U(bb + i, bb + kk), x[kk], acc);
      x[i] = (i <= c) ? acc * sm.rinv[bb + i] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) xs[bb + i][bb + c] = x[i];
  }
  __syncthreads();
#pragma unroll
  for (int h = 8; h < NU; h *= 2) {
    const int nb = NU / (2 * h), cnt = nb * h * h;
    for (int t = tid; t < cnt; t += 256) {  // T = U12 X22 (X22 upper: k <= c)
      const int blk = t / (h * h), r = (t / h) % h, c = t % h, o = blk * 2 * h;
      double acc = 0.0;
      for (int kk = 0; kk <= c; ++kk) acc = fma(U(o + r, o + h + kk), xs[o + h + kk][o + h + c], acc);
      tmp[o + r][o + h + c] = acc;
    }
    __syncthreads();
    for (int t = tid; t < cnt; t += 256) {  // X12 = -X11 T (X11 upper: kk >= r)
      const int blk = t / (h * h), r = (t / h) % h, c = t % h, o = blk * 2 * h;
      double acc = 0.0;
      for (int kk = r; kk < h; ++kk) acc = fma(xs[o + r][o + kk], tmp[o + kk][o + h + c], acc);
      xs[o + r][o + h + c] = -acc;
    }
    __syncthreads();
  }
}

// Fused panel step of chol_upper_rows (TG_CHOL_FUSED, the default): workgroup
// t factors the panel's diagonal block itself (every workgroup the same
// operations on the same block, so the same U11 and W in each) and forms its
// 64-column tile of the panel rows, P = W G12[:, tile], on FP64 MFMA, in
// place -- one launch where the potrf kernel, a GEMM launch and the gap
// between them were.  U11 is NOT written here (another workgroup may still
// be reading the block): chol_diag_kernel factors every panel's block again
// at the end (the blocks stay as they were factored: no later step of the
// factorisation writes them) and writes U11 and the pivot count.
__global__ __launch_bounds__(256) void chol_panel_kernel(double *__restrict__ U, int ldu, int p,
                                                         int pb, int c0, int n) {
  constexpr int RW = NU / 4;
  __shared__ PotrfSm sm;
  __shared__ double gs[NU][NU + 1];  // the tile of G12 (row l, column j)
  __shared__ double xs[NU][NU + 1];  // X = U11^-1
  __shared__ double xt[NU][NU + 1];  // the inverse's level products
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6, lr = lane >> 4, lc = lane & 15;
  const int col0 = c0 + NU * int(blockIdx.x);
  // the tile first (its loads in flight through the factorisation)
  double tv[NU * NU / 256];
#pragma unroll
  for (int u = 0; u < NU * NU / 256; ++u) {
    const int e = tid + 256 * u, r = e >> 6, cc = e & 63;
    tv[u] = U[size_t(p + min(r, pb - 1)) * ldu + min(col0 + cc, n - 1)];
  }
  double a[RW];
  (void)potrf_inv_block<4, false>(U + size_t(p) * ldu + p, ldu, pb, sm, a);
  __syncthreads();  // sm.ut / sm.rinv complete
  trinv64_blocked(sm, xs, xt);
#pragma unroll
  for (int u = 0; u < NU * NU / 256; ++u) {
    const int e = tid + 256 * u, r = e >> 6, cc = e & 63;
    gs[r][cc] = (r < pb) ? tv[u] : 0.0;
  }
  __syncthreads();
  // wave g: rows 16 g .. 16 g + 15 of P, four 16-column blocks, K = 64;
  // W = X^T restricted to the block's pb rows and columns
  doublex4 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) acc[cb] = doublex4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k0 = 0; k0 < NU; k0 += 4) {
    const int wi = 16 * g + lc, wk = k0 + lr;
    const double av = (wi < pb && wk < pb) ? xs[wk][wi] : 0.0;  // W[row][k] = X[k][row]
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
      acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, gs[k0 + lr][16 * cb + lc], acc[cb], 0, 0, 0);
  }
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = 16 * g + lr + 4 * q, cc = col0 + 16 * cb + lc;
      if (r < pb && cc < n) U[size_t(p + r) * ldu + cc] = acc[cb][q];
    }
}

// U11 of every panel of chol_upper_rows' fused form (one workgroup each, the
// panels' blocks as they were factored) and the count of non-positive pivots.
__global__ __launch_bounds__(256) void chol_diag_kernel(double *__restrict__ U, int ldu, int k,
                                                        int *__restrict__ info) {
  constexpr int RW = NU / 4;
  __shared__ PotrfSm sm;
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int p = NU * int(blockIdx.x), pb = min(NU, k - p);
  double a[RW];
  double *base = U + size_t(p) * ldu + p;
  const bool bad = potrf_inv_block<4, false>(base, ldu, pb, sm, a);
  if (threadIdx.x == 0 && bad) atomicAdd(info, 1);
  __syncthreads();  // every wave's reads of the block are done
#pragma unroll
  for (int q = 0; q < RW; ++q) {
    const int r = RW * g + q;
    if (r < pb && c < pb) base[size_t(r) * ldu + c] = c >= r ? a[q] : 0.0;
  }
}

// Row-panel triangular solve: X = Ubb^{-T} G[p:p+pb, c] for c in [c0, n).
// One thread per column; the column's pb unknowns live in LDS (xs[j][tid]).
__global__ __launch_bounds__(256) void trsm_rows_kernel(double *__restrict__ U, int ldu, int p, int pb,
                                                        int c0, int n) {
  __shared__ double ub[CB][CB + 1];
  __shared__ double xs[CB][256];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < CB * CB; idx += blockDim.x) {
    const int r = idx / CB, c = idx % CB;
    ub[r][c] = (r < pb && c < pb) ? U[size_t(p + r) * ldu + p + c] : (r == c ? 1.0 : 0.0);
  }
  const int c = c0 + blockIdx.x * blockDim.x + tid;
  const bool act = c < n;
  for (int j = 0; j < pb; ++j) xs[j][tid] = act ? U[size_t(p + j) * ldu + c] : 0.0;
  __syncthreads();
  for (int j = 0; j < pb; ++j) {
    double v = xs[j][tid];
    for (int l = 0; l < j; ++l) v -= ub[l][j] * xs[l][tid];
    xs[j][tid] = v / ub[j][j];
  }
  if (act)
    for (int j = 0; j < pb; ++j) U[size_t(p + j) * ldu + c] = xs[j][tid];
}

__global__ void zero_lower_kernel(double *__restrict__ U, int ldu, int k) {
  const int r = blockIdx.y;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < r && c < k; c += gridDim.x * blockDim.x)
    U[size_t(r) * ldu + c] = 0.0;
}


// Right-looking blocked upper Cholesky of the first k rows of the symmetric
// n x n matrix in U (upper triangle read): U[:k, :] <- R with R^T R = G
// restricted to those rows (k = n: the full factor).  NU-row panels: the
// diagonal block and its inverse (potrf_inv_4w_kernel), the panel rows as
// one MFMA GEMM U12 = U11^-T G12, the trailing update as a second GEMM.
// info[0] counts non-positive pivots.
// Diagonal-block factor + inverse: the four-wave kernel.
static void launch_potrf_inv(hipStream_t st, double *U, int ldu, int p, int pb, double *Wb,
                             int *info) {
  hipLaunchKernelGGL(potrf_inv_4w_kernel<4>, dim3(1), dim3(256), 0, st, U, ldu, p, pb, Wb, info);
}

// Two-level blocking: NU-row panels inside strips of CS = 256 rows.  A
// panel's rank-NU update only reaches the rest of its strip; the rows below
// the strip get one rank-CS update per strip (a quarter of the passes over
// the trailing matrix, and at K = 256 the update is MFMA-bound instead of
// HBM-bound: at k = 12,288 the 192 rank-64 updates streamed ~150 GB).  When
// k == n the trailing matrix is symmetric and that update is a SYRK on the
// lower tiles, mirrored (half the flops of the square).  The strip update
// writes the whole trailing square (lower tiles mirrored): later panels read
// only its upper triangle.
constexpr int CS = 256;

hipError_t chol_upper_rows(hipStream_t st, double *U, int ldu, int k, int n, double *Wb,
                           int *info) {
  // (a depth-1 look-ahead on a side stream measured +0.4 ms: the event
  // waits cost more than the overlap; removed)
  // TG_CHOL_FUSED=0: the potrf kernel and a GEMM launch per panel (the
  // panel's U11 written at once) instead of chol_panel_kernel + chol_diag_kernel
  const char *cf = getenv("TG_CHOL_FUSED");  // development switch, read per call
  const bool fused = !(cf && cf[0] == '0');
  for (int s0 = 0; s0 < k; s0 += CS) {
    const int se = std::min(k, s0 + CS);
    for (int p = s0; p < se; p += NU) {
      const int pb = std::min(NU, se - p);
      const int c0 = p + pb;
      hipError_t e = hipSuccess;
      if (fused) {
        if (c0 < n)
          hipLaunchKernelGGL(chol_panel_kernel, dim3(tg::cdiv(n - c0, NU)), dim3(256), 0, st, U, ldu,
                             p, pb, c0, n);
        if ((e = hipGetLastError()) != hipSuccess) return e;
      } else {
        launch_potrf_inv(st, U, ldu, p, pb, Wb, info);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (c0 < n) {
          // in place: one 64-row tile covers the panel's rows, so each workgroup
          // reads its columns of G12 fully before writing them
          double *P = U + size_t(p) * ldu + c0;
          e = tg::dgemm(st, false, false, pb, n - c0, pb, 1.0, Wb, NU, P, ldu, 0.0, P, ldu);
          if (e != hipSuccess) return e;
        }
      }
      if (c0 < se) {  // the rest of the strip
        const double *P = U + size_t(p) * ldu + c0;
        e = tg::dgemm(st, true, false, se - c0, n - c0, pb, -1.0, P, ldu, P, ldu, 1.0,
                      U + size_t(c0) * ldu + c0, ldu);
        if (e != hipSuccess) return e;
      }
    }
    if (se < k) {  // rows below the strip: one rank-(se - s0) update
      const double *Q = U + size_t(s0) * ldu + se;
      const hipError_t e =
          k == n ? tg::dsyrk_tn(st, n - se, se - s0, -1.0, Q, ldu, 1.0, U + size_t(se) * ldu + se,
                                ldu)
                 : tg::dgemm(st, true, false, k - se, n - se, se - s0, -1.0, Q, ldu, Q, ldu, 1.0,
                             U + size_t(se) * ldu + se, ldu);
      if (e != hipSuccess) return e;
    }
  }
  if (fused && k > 0) {
    hipLaunchKernelGGL(chol_diag_kernel, dim3(tg::cdiv(k, NU)), dim3(256), 0, st, U, ldu, k, info);
    return hipGetLastError();
  }
  return hipSuccess;
}

// ---------------------------------------------------------------------------
// GPTQ comparator factor (process_hessian, gptq_utils.py:129-165):
// R = chol_upper(inv(H_p + damp I)), H_p = H[perm][:, perm].  With J the
// reversal, chol_upper(J H_p J) = U' gives H_p = Ut Ut^T for the upper
// Ut = J U'^T J, hence inv(H_p) = Ut^-T Ut^-1 and R = Ut^-1 = J (U'^-1)^T J:
// one Cholesky and one triangular inverse instead of the reference's
// cholesky -> cholesky_inverse -> cholesky (same matrix, other rounding).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void diag_mean_kernel(const double *__restrict__ H, int64_t ldh,
                                                        int n, double *__restrict__ mean) {
  __shared__ double part[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += H[i * ldh + i];
  part[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += part[i];  // fixed order: deterministic
    t /= double(n);
    mean[0] = (t == 0.0) ? 1.0 : t;              // :144-145
  }
}

// A[i][j] = H[p(n-1-i)][p(n-1-j)] + (i == j) damp * mean
__global__ void flip_damp_kernel(const double *__restrict__ H, int64_t ldh, int n,
                                 const int64_t *__restrict__ perm, double damp,
                                 const double *__restrict__ mean, double *__restrict__ A) {
  // Entry (i, j) of A = J H_p J is H_p[n-1-i][n-1-j]; it is always read from
  // H_p's LOWER triangle (row n-1-min(i,j) >= column n-1-max(i,j)), the only
  // triangle the reference's torch.linalg.cholesky(H_damped) reads
  // (gptq_utils.py:152), so an H that is not bit-symmetric factors the same
  // way.  A itself is then exactly symmetric, whichever triangle
  // chol_upper_rows' panels and strip SYRKs read.
  const int i = blockIdx.y;
  const double dm = damp * mean[0];
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    const int r = n - 1 - min(i, j), c = n - 1 - max(i, j);
    const int64_t pr = perm ? perm[r] : r, pc = perm ? perm[c] : c;
    double v = H[pr * ldh + pc];
    if (i == j) v += dm;
    A[int64_t(i) * n + j] = v;
  }
}

// Y_bb = U_bb^-1 for every NU x NU diagonal block b (one workgroup each);
// the rest of Y is left to the caller (zeroed, then filled by GEMMs).
__global__ __launch_bounds__(256) void trinv_diag_kernel(const double *__restrict__ U, int ldu,
                                                         int n, double *__restrict__ Y, int ldy) {
  __shared__ double a[NU][NU + 1];
  __shared__ double x[NU][NU + 1];
  const int p = blockIdx.x * NU, pb = min(NU, n - p), tid = threadIdx.x;
  for (int idx = tid; idx < NU * NU; idx += blockDim.x) {
    const int r = idx / NU, c = idx % NU;
    a[r][c] = (r < pb && c < pb) ? (c >= r ? U[size_t(p + r) * ldu + p + c] : 0.0)
                                 : (r == c ? 1.0 : 0.0);
  }
  __syncthreads();
  const int c = tid >> 2, part = tid & 3;
  for (int i = NU - 1; i >= 0; --i) {
    double sacc = 0.0;
    if (i < c)
      for (int l = i + 1 + part; l <= c; l += 4) sacc += a[i][l] * x[l][c];
    sacc += __shfl_xor(sacc, 1);
    sacc += __shfl_xor(sacc, 2);
    if (part == 0) x[i][c] = i > c ? 0.0 : ((i == c ? 1.0 : 0.0) - sacc) / a[i][i];
    __syncthreads();
  }
  for (int idx = tid; idx < pb * pb; idx += blockDim.x) {
    const int r = idx / pb, cc = idx % pb;
    Y[size_t(p + r) * ldy + p + cc] = x[r][cc];
  }
}

// Off-diagonal blocks of Y = U^-1 (upper; the NU x NU diagonal blocks are
// already in Y, everything below the diagonal is zero).  Bottom-up: at block
// size b = NU, 2NU, ... each pair of adjacent solved blocks merges with
// Y12 = -(Y11 U12) Y22.  All full-size pairs of a level are independent and
// go out as two batched GEMMs, which skip the zero triangles of Y11 and Y22
// (half their flops); a pair whose second block is the ragged tail gets two
// plain GEMMs.  T holds >= n*n/4 doubles.
// bmax: stop before merging blocks of bmax rows (the diagonal bmax x bmax
// blocks of Y are then the inverses of U's, the rest untouched).
hipError_t trinv_offdiag(hipStream_t st, const double *U, int ldu, double *Y, int ldy, int n,
                         double *T, int bmax = 1 << 30) {
  for (int b = NU; b < n && b < bmax; b *= 2) {
    const int nblk = tg::cdiv(n, b), npair = nblk / 2;
    const bool ragged = npair > 0 && 2 * npair * b > n;
    const int nfull = ragged ? npair - 1 : npair;
    hipError_t e = hipSuccess;
    if (nfull > 0) {
      const int64_t bb = int64_t(b) * b, dy = int64_t(ldy) + 1, du = int64_t(ldu) + 1;
      const tg::ChunkSpec c1{2 * b, nfull, 2 * b * nfull, dy, 0, du, 0, 0, bb, b, b, b};
      e = tg::dgemm_chunked(st, false, false, c1, 1.0, Y, ldy, U + b, ldu, 0.0, T, b, 1);
      if (e != hipSuccess) return e;
      const tg::ChunkSpec c2{2 * b, nfull, 2 * b * nfull, 0, bb, dy, 0, dy, 0, b, b, b};
      e = tg::dgemm_chunked(st, false, false, c2, -1.0, T, b, Y + size_t(b) * ldy + b, ldy, 0.0,
                            Y + b, ldy, 2);
      if (e != hipSuccess) return e;
    }
    if (ragged) {
      const size_t s = size_t(2) * (npair - 1) * b;
      const int b2 = n - int(s) - b;
      e = tg::dgemm(st, false, false, b, b2, b, 1.0, Y + s * ldy + s, ldy, U + s * ldu + s + b,
                    ldu, 0.0, T, b2);
      if (e != hipSuccess) return e;
      e = tg::dgemm(st, false, false, b, b2, b2, -1.0, T, b2, Y + (s + b) * ldy + s + b, ldy, 0.0,
                    Y + s * ldy + s + b, ldy);
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

// R[i][j] = Y[n-1-j][n-1-i] (j >= i), 0 below the diagonal
__global__ void flip_transpose_kernel(const double *__restrict__ Y, int n, double *__restrict__ R,
                                      int64_t ldr) {
  const int i = blockIdx.y;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
    R[i * ldr + j] = j >= i ? Y[int64_t(n - 1 - j) * n + (n - 1 - i)] : 0.0;
}

__global__ void identity_kernel(int n, double *__restrict__ R, int64_t ldr) {
  const int i = blockIdx.y;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
    R[i * ldr + j] = i == j ? 1.0 : 0.0;
}

// ---------------------------------------------------------------------------
// Conditioning guard of the Gram-matrix (CholeskyQR) factors of U.
// tg_u_factor and tg_u_factor_rx take R from the Cholesky factor of a Gram
// matrix Y^T Y, which squares Y's condition number (the reference runs a
// Householder QR, gptq_utils.py:120).  After the first Cholesky the host reads
// the factor's info count and diagonal range; when a pivot broke down, or
// (max/min diag)^2 * eps puts the factor's error above ~1e-9, the factor is
// refined by CholeskyQR passes on the explicit Q = Y R^-1 (CholeskyQR2), with
// a shifted first factorisation when the plain one broke down (shifted
// CholeskyQR3: G + s I, s = 11 (k^2 + k (k+1)) u ||Y||_F^2).  When that
// refinement breaks down too (cond(Y) past ~3e13), R comes from a Householder
// QR of Y itself (hqr.hip, householder_r below; switch TG_U_QR).
// ---------------------------------------------------------------------------
// out[0] = max |d_i|, out[1] = min d_i (0 when any is non-positive or not
// finite), diagonal of the k x k upper factor U
__global__ __launch_bounds__(256) void diag_range_kernel(const double *__restrict__ U, int64_t ldu,
                                                         int k, double *__restrict__ out) {
  __shared__ double mx[256], mn[256];
  double a = 0.0, b = DBL_MAX;
  for (int i = threadIdx.x; i < k; i += 256) {
    const double d = U[i * ldu + i];
    const bool ok = d > 0.0 && d <= DBL_MAX;
    a = ok ? fmax(a, d) : a;
    b = ok ? fmin(b, d) : 0.0;
  }
  mx[threadIdx.x] = a;
  mn[threadIdx.x] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      mx[threadIdx.x] = fmax(mx[threadIdx.x], mx[threadIdx.x + s]);
      mn[threadIdx.x] = fmin(mn[threadIdx.x], mn[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = mx[0];
    out[1] = mn[0];
  }
}

// out[0] = trace of the k x k matrix G (fixed summation order)
__global__ __launch_bounds__(256) void diag_sum_kernel(const double *__restrict__ G, int64_t ldg,
                                                       int k, double *__restrict__ out) {
  __shared__ double part[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < k; i += 256) acc += G[i * ldg + i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = part[0];
}

__global__ void add_diag_kernel(double *__restrict__ G, int64_t ldg, int k, double s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k) G[i * ldg + i] += s;
}

struct CholStat {
  double dmax, dmin, trace;
  int info;
};

// stats[0..2] = {max diag, min diag, trace}, info -> host (one sync)
static hipError_t read_stat(hipStream_t st, const double *stats, const int *info, CholStat &h) {
  double v[3];
  hipError_t e = hipMemcpyAsync(v, stats, sizeof(v), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(&h.info, info, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  h.dmax = v[0];
  h.dmin = v[1];
  h.trace = v[2];
  return e;
}

// 0: never refine, 1: always refine, 2 (default): refine when the guard asks
static int refine_mode() {
  const char *e = getenv("TG_U_REFINE");
  return (e && e[0] == '0') ? 0 : (e && e[0] == '1') ? 1 : 2;
}

// the first factor is not trusted: breakdown (always handled), or
// (dmax/dmin)^2 eps > 1e-9 (TG_U_REFINE=0 / 1 disable / force this part)
static bool needs_refine(const CholStat &h) {
  if (h.info > 0 || !(h.dmin > 0.0)) return true;
  const int mode = refine_mode();
  if (mode != 2) return mode == 1;
  const double r = h.dmax / h.dmin;
  return r * r * DBL_EPSILON > 1e-9;
}

// Y = R^-1 (k x k upper, ld k); T: trinv_offdiag scratch
static hipError_t trinv(hipStream_t st, const double *R, int ldr, int k, double *Y, double *T) {
  hipError_t e = hipMemsetAsync(Y, 0, sizeof(double) * size_t(k) * k, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(trinv_diag_kernel, dim3(tg::cdiv(k, NU)), dim3(256), 0, st, R, ldr, k, Y, k);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return trinv_offdiag(st, R, ldr, Y, k, k, T);
}

static hipError_t zero_lower(hipStream_t st, double *U, int ldu, int k) {
  hipLaunchKernelGGL(zero_lower_kernel, dim3(tg::cdiv(k, 256) < 16 ? tg::cdiv(k, 256) : 16, k),
                     dim3(256), 0, st, U, ldu, k);
  return hipGetLastError();
}

// Scratch of the refinement: Ri, Q, G (k x k each), T (trinv), stats.
struct RefineWs {
  double *Ri, *Q, *G, *T, *stats;
};

// Which factor the last U-factor call of this thread returned
// (tg_u_factor_last_path): 0 Gram, 1 Gram + CholeskyQR refinement, 2 Householder.
thread_local int g_u_path = 0;
// refine_factor's status when the refinement gives up (as opposed to a failed
// HIP call); the entry points return it as hipErrorUnknown
constexpr int REFINE_BROKE = -1000;
static int refine_status(int e) { return e == REFINE_BROKE ? int(hipErrorUnknown) : e; }

// Shifted first factor: R (k x k, ld k) = chol(Y^T Y + s I), s from trace(Y^T Y).
static int shifted_factor(hipStream_t st, const double *Y, int64_t ldy, int k, double *R,
                          RefineWs &w, double *Wb, int *info, CholStat &h) {
  TG_HIP(tg::dsyrk_tn(st, k, k, 1.0, Y, ldy, 0.0, R, k));
  hipLaunchKernelGGL(diag_sum_kernel, dim3(1), dim3(256), 0, st, R, int64_t(k), k, w.stats + 2);
  TG_LAUNCHED();
  TG_HIP(read_stat(st, w.stats, info, h));
  const double kk = double(k);
  const double s = 11.0 * (kk * kk + kk * (kk + 1.0)) * (DBL_EPSILON / 2) * h.trace;
  hipLaunchKernelGGL(add_diag_kernel, dim3(tg::cdiv(k, 256)), dim3(256), 0, st, R, int64_t(k), k, s);
  TG_LAUNCHED();
  TG_HIP(hipMemsetAsync(info, 0, sizeof(int), st));
  TG_HIP(chol_upper_rows(st, R, k, k, k, Wb, info));
  TG_HIP(zero_lower(st, R, k, k));
  hipLaunchKernelGGL(diag_range_kernel, dim3(1), dim3(256), 0, st, R, int64_t(k), k, w.stats);
  TG_LAUNCHED();
  TG_HIP(read_stat(st, w.stats, info, h));
  if (h.info > 0 || !(h.dmin > 0.0)) {
    tg::set_error("U factor: shifted Cholesky of the Gram matrix broke down (%d pivots; "
                  "input not of full rank k = %d)", h.info, k);
    return REFINE_BROKE;
  }
  return 0;
}

// One CholeskyQR pass: Q = Y R^-1, Q^T Q = R'^T R', R <- R' R.
static int cholqr_pass(hipStream_t st, const double *Y, int64_t ldy, int k, double *R,
                       RefineWs &w, double *Wb, int *info) {
  TG_HIP(trinv(st, R, k, k, w.Ri, w.T));
  TG_HIP(tg::dgemm(st, false, false, k, k, k, 1.0, Y, ldy, w.Ri, k, 0.0, w.Q, k));
  TG_HIP(tg::dsyrk_tn(st, k, k, 1.0, w.Q, k, 0.0, w.G, k));
  TG_HIP(hipMemsetAsync(info, 0, sizeof(int), st));
  TG_HIP(chol_upper_rows(st, w.G, k, k, k, Wb, info));
  TG_HIP(zero_lower(st, w.G, k, k));
  TG_HIP(tg::dgemm(st, false, false, k, k, k, 1.0, w.G, k, R, k, 0.0, w.Ri, k));  // R' R
  TG_HIP(hipMemcpyAsync(R, w.Ri, sizeof(double) * size_t(k) * k, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(diag_range_kernel, dim3(1), dim3(256), 0, st, R, int64_t(k), k, w.stats);
  TG_LAUNCHED();
  CholStat h{};
  TG_HIP(read_stat(st, w.stats, info, h));
  if (h.info > 0 || !(h.dmin > 0.0)) {
    tg::set_error("U factor: CholeskyQR refinement broke down (%d pivots, k = %d)", h.info, k);
    return REFINE_BROKE;
  }
  return 0;
}

// Refined R (k x k, ld k) of Y (k x k, ld ldy), given the first factor in R
// and its statistics h: shifted restart on breakdown, then 1 (2 after a
// shift) CholeskyQR passes.
static int refine_factor(hipStream_t st, const double *Y, int64_t ldy, int k, double *R,
                         RefineWs &w, double *Wb, int *info, CholStat h) {
  int passes = 1;
  if (h.info > 0 || !(h.dmin > 0.0)) {
    const int e = shifted_factor(st, Y, ldy, k, R, w, Wb, info, h);
    if (e != 0) return e;
    passes = 2;
  }
  for (int p = 0; p < passes; ++p) {
    const int e = cholqr_pass(st, Y, ldy, k, R, w, Wb, info);
    if (e != 0) return e;
  }
  return 0;
}

// TG_U_QR (read per call): 0 auto (Gram form, Householder QR when its
// refinement breaks down), 1 gram (no fallback), 2 householder (no Gram attempt)
static int uqr_mode() {
  const char *e = getenv("TG_U_QR");
  if (e && strcmp(e, "gram") == 0) return 1;
  if (e && strcmp(e, "householder") == 0) return 2;
  return 0;
}

// Householder fallback (hqr.hip): Y (k x n, ld ldy) becomes its R in place.
// No Gram matrix is formed, so cond(Y) is not squared.  The scratch is the
// refinement's Ri .. T, contiguous in the arena and free at this point.
static int householder_r(hipStream_t st, double *Y, int64_t ldy, int k, int n, RefineWs &w) {
  const size_t bytes = size_t(reinterpret_cast<char *>(w.stats) - reinterpret_cast<char *>(w.Ri));
  if (const int e = tg::hqr_r(st, Y, ldy, k, n, w.Ri, bytes)) return e;
  hipLaunchKernelGGL(diag_range_kernel, dim3(1), dim3(256), 0, st, Y, ldy, k, w.stats);
  TG_LAUNCHED();
  double v[2];
  TG_HIP(hipMemcpyAsync(v, w.stats, sizeof(v), hipMemcpyDeviceToHost, st));
  TG_HIP(hipStreamSynchronize(st));
  if (!(v[1] > 0.0)) {
    tg::set_error("U factor: Householder QR broke down (zero or non-finite diagonal entry; "
                  "input not of full rank k = %d)", k);
    return int(hipErrorUnknown);
  }
  g_u_path = 2;
  return 0;
}

// R (k x k, ld k) of Yq (k x k, ld k) at the refinement point of the R_x
// forms: CholeskyQR refinement of the first factor in Rq, or the Householder R
// of Yq (in place, then copied to Rq) when that breaks down or mode = 2.
static int refine_or_householder(hipStream_t st, double *Yq, int k, double *Rq, RefineWs &rw,
                                 double *Wb, int *info, const CholStat &h, int mode) {
  if (mode != 2) {
    const int e = refine_factor(st, Yq, k, k, Rq, rw, Wb, info, h);
    if (e == 0) g_u_path = 1;
    if (e != REFINE_BROKE || mode == 1) return refine_status(e);
  }
  if (const int e = householder_r(st, Yq, k, k, k, rw)) return e;
  TG_HIP(hipMemcpyAsync(Rq, Yq, sizeof(double) * size_t(k) * k, hipMemcpyDeviceToDevice, st));
  return 0;
}

}  // namespace

extern "C" int tg_u_factor_last_path(void) { return g_u_path; }


template <class Ar>
static void refine_layout(Ar &ar, int k, RefineWs *w) {
  RefineWs d{};
  RefineWs &q = w ? *w : d;
  const size_t h = size_t(NU) * ((tg::cdiv(k, NU) + 1) / 2);
  auto t = [&](double *&dst, size_t cnt) { dst = ar.template take<double>(cnt); };
  t(q.Ri, size_t(k) * k);
  t(q.Q, size_t(k) * k);
  t(q.G, size_t(k) * k);
  t(q.T, h * h);
  t(q.stats, 8);
}

template <class Ar>
static void ufac_layout(Ar &ar, int n, int k, double **A, int **info, double **Wb, double **Rk,
                        RefineWs *w) {
  auto t = [&](auto *&dst, size_t cnt) {
    using T = std::remove_reference_t<decltype(*dst)>;
    dst = ar.template take<T>(cnt);
  };
  double *d[3];
  int *i0;
  t(A ? *A : d[0], size_t(k) * n);
  t(info ? *info : i0, 16);
  t(Wb ? *Wb : d[1], NU * NU);
  t(Rk ? *Rk : d[2], size_t(k) * k);
  refine_layout(ar, k, w);
}

extern "C" size_t tg_ufactor_workspace_size(int n, int k) {
  tg::Sizer s;
  ufac_layout(s, n, k, nullptr, nullptr, nullptr, nullptr, nullptr);
  return s.off + 256;
}

extern "C" int tg_u_factor(void *stream, const double *Vh, int ldv, const double *S,
                           const int64_t *perm, int n, int k, double *U, int ldu, void *ws,
                           size_t ws_bytes) {
  TG_ARG(Vh, 2, "null Vh");
  TG_ARG(ldv >= n, 3, "ldv < n");
  TG_ARG(S, 4, "null S");
  TG_ARG(perm, 5, "null perm");
  TG_ARG(n >= 1, 6, "n < 1");
  TG_ARG(k >= 1 && k <= n, 7, "k must be in [1, n]");
  TG_ARG(U, 8, "null U");
  TG_ARG(ldu >= n, 9, "ldu < n");
  hipStream_t st = (hipStream_t)stream;
  tg::Arena ar(ws, ws_bytes);
  double *A, *Wb, *Rk;
  int *info;
  RefineWs rw{};
  ufac_layout(ar, n, k, &A, &info, &Wb, &Rk, &rw);
  TG_WS(ar);
  g_u_path = 0;
  const int mode = uqr_mode();
  TG_HIP(hipMemsetAsync(info, 0, sizeof(int), st));
  hipLaunchKernelGGL(gather_scale_kernel, dim3(tg::cdiv(n, 256) < 16 ? tg::cdiv(n, 256) : 16, k),
                     dim3(256), 0, st, Vh, ldv, S, perm, n, A);
  TG_LAUNCHED();
  if (mode != 2) {
    // G[:k, :] = A[:, :k]^T A   (k x n) into U
    TG_HIP(tg::dgemm(st, true, false, k, n, k, 1.0, A, n, A, n, 0.0, U, ldu));
    TG_HIP(chol_upper_rows(st, U, ldu, k, n, Wb, info));
    TG_HIP(zero_lower(st, U, ldu, k));
    hipLaunchKernelGGL(diag_range_kernel, dim3(1), dim3(256), 0, st, U, int64_t(ldu), k, rw.stats);
    TG_LAUNCHED();
    CholStat h{};
    TG_HIP(read_stat(st, rw.stats, info, h));
    if (!needs_refine(h)) return 0;
    // Refined: R11 by CholeskyQR passes on A1 = A[:, :k], then R12 = Q^T A2
    // with the explicit Q = A1 R11^-1 (not R11^-T G12, whose error grows with
    // cond(A1)^2).
    if (h.info == 0 && h.dmin > 0.0)
      TG_HIP(hipMemcpy2DAsync(Rk, sizeof(double) * k, U, sizeof(double) * ldu, sizeof(double) * k,
                              k, hipMemcpyDeviceToDevice, st));
    const int e = refine_factor(st, A, n, k, Rk, rw, Wb, info, h);
    if (e == 0) {
      TG_HIP(trinv(st, Rk, k, k, rw.Ri, rw.T));
      TG_HIP(tg::dgemm(st, false, false, k, k, k, 1.0, A, n, rw.Ri, k, 0.0, rw.Q, k));
      TG_HIP(hipMemcpy2DAsync(U, sizeof(double) * ldu, Rk, sizeof(double) * k, sizeof(double) * k,
                              k, hipMemcpyDeviceToDevice, st));
      if (n > k)
        TG_HIP(tg::dgemm(st, true, false, k, n - k, k, 1.0, rw.Q, k, A + k, n, 0.0, U + k, ldu));
      g_u_path = 1;
      return 0;
    }
    if (e != REFINE_BROKE || mode == 1) return refine_status(e);
  }
  // Householder QR of the gathered A in place (refine_factor left it intact):
  // the trailing columns get Q^T A2 from the reflectors themselves.
  if (const int e = householder_r(st, A, n, k, n, rw)) return e;
  TG_HIP(hipMemcpy2DAsync(U, sizeof(double) * ldu, A, sizeof(double) * n, sizeof(double) * n, k,
                          hipMemcpyDeviceToDevice, st));
  return 0;
}

// U from R_x alone (complement path, no kept eigenvectors):
// P^T H_k P = L L^T with L = R_x^T (n x k, full column rank), so
// P^T H_k^+ P = L (L^T L)^-2 L^T = A^T A with A = S^-1 R_x, S = R_x R_x^T,
// and U is the R factor of A (positive diagonal).
//
// Default (one serial Cholesky).  With R_x = [R11 R12] (R11 k x k upper
// triangular, invertible) and C = R11^-1 R12:
//   S = R11 (I + C C^T) R11^T,  Z := R11^-1 S = R11^T + C R12^T,
//   A = S^-1 R_x = Z^-1 R11^-1 R_x = Z^-1 [I C].
// With N = Z Z^T = V V^T (V upper triangular, positive diagonal),
//   A^T A = [I C]^T N^-1 [I C] = (V^-1 [I C])^T (V^-1 [I C]),
// and V^-1 [I C] is upper trapezoidal with positive diagonal, so by
// uniqueness of the R factor  U = [V^-1, V^-1 C].  V comes from the upper
// Cholesky of the reversed N' = J N J = R^T R:  V = J R^T J, V^-1 = J R^-T J.
// Work: two triangular inverses (parallel recursive GEMMs), four GEMMs and
// ONE k x k blocked Cholesky, against two Choleskys (one over k x n rows) for
// the form below (TG_URX_TWOCHOL=1): S = T^T T, Y = T^-1, A = Y (Y^T R_x),
// U = first k rows of the upper Cholesky of A^T A.
// N has the conditioning of A[:, :k]^T A[:, :k], the same matrix the second
// Cholesky of the two-Cholesky form factors.
template <class Ar>
static void urx_layout(Ar &ar, int n, int k, double **S, double **Y, double **Bm, double **A,
                       double **Tt, double **Wb, int **info, double **Rq, RefineWs *rw) {
  const size_t h = size_t(NU) * ((tg::cdiv(k, NU) + 1) / 2);
  auto t = [&](auto *&dst, size_t cnt) {
    using T = std::remove_reference_t<decltype(*dst)>;
    dst = ar.template take<T>(cnt);
  };
  double *d[7];
  int *i0;
  t(S ? *S : d[0], size_t(k) * k);
  t(Y ? *Y : d[1], size_t(k) * k);
  t(Bm ? *Bm : d[2], size_t(k) * n);
  t(A ? *A : d[3], size_t(k) * n);
  t(Tt ? *Tt : d[4], h * h);
  t(Wb ? *Wb : d[5], size_t(NU) * NU);
  t(info ? *info : i0, 16);
  t(Rq ? *Rq : d[6], size_t(k) * k);
  refine_layout(ar, k, rw);
}


// N'[i][j] = N[k-1-i][k-1-j]
__global__ void flip_both_kernel(const double *__restrict__ N, int k, double *__restrict__ Np) {
  const int i = blockIdx.y;
  const double *src = N + size_t(k - 1 - i) * k + (k - 1);
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < k; j += gridDim.x * blockDim.x)
    Np[size_t(i) * k + j] = src[-j];
}

extern "C" size_t tg_ufactor_rx_workspace_size(int n, int k) {
  tg::Sizer s;
  urx_layout(s, n, k, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
             nullptr);
  return s.off + 256;
}

// C = R11^-1 B for the upper-triangular R11 (k x k, ld ldr; its strict lower
// triangle zero) and B (k x m, ld ldr): back substitution by TB-row blocks
// from the bottom, block i = Dinv_i (Cw_i) then Cw[0:p] -= R11[0:p, i] C_i;
// Dinv (ld ldd) holds the inverses of the TB x TB diagonal blocks.
// Cw: k x m scratch (ld m); C: k x m (ld m).  k^2 m flops against the
// explicit R11^-1's k^3 / 3 (the near-full-rank layers' m = n - k is tiny).
constexpr int TB = 256;
static int trsm_upper_blocks(hipStream_t st, const double *R, int ldr, int k, const double *B,
                             int m, const double *Dinv, int ldd, double *Cw, double *C, int ldc) {
  TG_HIP(hipMemcpy2DAsync(Cw, sizeof(double) * ldc, B, sizeof(double) * ldr, sizeof(double) * m,
                          k, hipMemcpyDeviceToDevice, st));
  for (int bi = tg::cdiv(k, TB) - 1; bi >= 0; --bi) {
    const int p = bi * TB, pb = std::min(TB, k - p);
    TG_HIP(tg::dgemm(st, false, false, pb, m, pb, 1.0, Dinv + size_t(p) * ldd + p, ldd,
                     Cw + size_t(p) * ldc, ldc, 0.0, C + size_t(p) * ldc, ldc));
    if (p > 0)
      TG_HIP(tg::dgemm(st, false, false, p, m, pb, -1.0, R + p, ldr, C + size_t(p) * ldc, ldc, 1.0,
                       Cw, ldc));
  }
  return 0;
}

// The small-m form of the U factor (below): m * 16 <= k by default;
// TG_URX_SMALLM=0 / 1 forces the explicit-inverse form / this one.
static bool urx_small_m(int k, int m) {
  const char *e = getenv("TG_URX_SMALLM");
  if (e) return e[0] == '1';
  return int64_t(m) * 16 <= int64_t(k);
}

// Stages of the explicit form (below), shared with the column-sharded entry
// points (tg_urx_c / tg_urx_u11 / tg_urx_u12, gptq_svd_amd.dist.
// u_factor_rx_sharded): each column of C = R11^-1 R12 and of U12 = V^-1 C
// depends on its own column of R12 / C only (block back substitution and
// GEMMs with a fixed k order per entry), so a rank computing a column block
// gets the single-call values bit for bit.
// (a) the 256-block diagonal inverses of R11 into Yr (k x k, zeroed first)
static int urx_diag_inverses(hipStream_t st, const double *Rx, int ldr, int k, double *Yr,
                             double *Tt) {
  TG_HIP(hipMemsetAsync(Yr, 0, sizeof(double) * size_t(k) * k, st));
  hipLaunchKernelGGL(trinv_diag_kernel, dim3(tg::cdiv(k, NU)), dim3(256), 0, st, Rx, ldr, k, Yr,
                     k);
  TG_LAUNCHED();
  TG_HIP(trinv_offdiag(st, Rx, ldr, Yr, k, k, Tt, TB));
  return 0;
}
// (b) from the full C (k x m, ld ldc): Z^T = R11 + R12 C^T, N = Z Z^T, the
// Cholesky of N' = J N J (refined when ill-conditioned) and U11 = V^-1 into
// U; Yr, ZT, Nm, Rq: k x k scratch
static int urx_u11_from_c(hipStream_t st, const double *Rx, int ldr, int n, int k, const double *C,
                          int ldc, double *U, int ldu, double *Yr, double *ZT, double *Nm,
                          double *Rq, double *Tt, double *Wb, int *info, RefineWs &rw) {
  const int m = n - k;
  const dim3 gk(tg::cdiv(k, 256) < 16 ? tg::cdiv(k, 256) : 16, k);
  auto form_zt = [&](bool scratch_free) -> int {  // Z^T = R11 + R12 C^T
    TG_HIP(hipMemcpy2DAsync(ZT, sizeof(double) * k, Rx, sizeof(double) * ldr, sizeof(double) * k,
                            k, hipMemcpyDeviceToDevice, st));
    if (m <= 0) return 0;
    // the DGEMM stages 16-byte vectors only from 16-byte-aligned rows: with
    // an odd k R12's rows start mid-vector, so it is copied to an even-ld
    // buffer first (Y, when the caller says it is not live; C has an even
    // ld already)
    const int mp = m + (m & 1);
    const bool pad = scratch_free && ((k & 1) || (ldr & 1)) && mp <= k;
    if (pad) {
      double *R12p = Yr;
      TG_HIP(hipMemcpy2DAsync(R12p, sizeof(double) * mp, Rx + k, sizeof(double) * ldr,
                              sizeof(double) * m, k, hipMemcpyDeviceToDevice, st));
      TG_HIP(tg::dgemm(st, false, true, k, k, m, 1.0, R12p, mp, C, ldc, 1.0, ZT, k));
    } else {
      TG_HIP(tg::dgemm(st, false, true, k, k, m, 1.0, Rx + k, ldr, C, ldc, 1.0, ZT, k));
    }
    return 0;
  };
  if (const int e = form_zt(true)) return e;
  const int mode = uqr_mode();
  CholStat h{};
  if (mode != 2) {
    TG_HIP(tg::dsyrk_tn(st, k, k, 1.0, ZT, k, 0.0, Nm, k));         // N = Z Z^T
    hipLaunchKernelGGL(flip_both_kernel, gk, dim3(256), 0, st, Nm, k, Rq);  // N' = J N J
    TG_LAUNCHED();
    TG_HIP(chol_upper_rows(st, Rq, k, k, k, Wb, info));               // N' = R^T R
    hipLaunchKernelGGL(diag_range_kernel, dim3(1), dim3(256), 0, st, Rq, int64_t(k), k, rw.stats);
    TG_LAUNCHED();
    TG_HIP(read_stat(st, rw.stats, info, h));
  }
  if (mode == 2 || needs_refine(h)) {
    double *Yq = Nm;
    if (mode != 2) TG_HIP(zero_lower(st, Rq, k, k));
    hipLaunchKernelGGL(flip_both_kernel, gk, dim3(256), 0, st, ZT, k, Yq);
    TG_LAUNCHED();
    const int e = refine_or_householder(st, Yq, k, Rq, rw, Wb, info, h, mode);
    if (e != 0) return e;
  }
  TG_HIP(trinv(st, Rq, k, k, Yr, Tt));                              // Yr = R^-1
  hipLaunchKernelGGL(flip_transpose_kernel, gk, dim3(256), 0, st, Yr, k, U, int64_t(ldu));
  TG_LAUNCHED();                                                    // U11 = V^-1 = J R^-T J
  return 0;
}

extern "C" int tg_u_factor_rx(void *stream, const double *Rx, int ldr, int n, int k, double *U,
                              int ldu, void *ws, size_t ws_bytes) {
  TG_ARG(Rx, 2, "null Rx");
  TG_ARG(ldr >= n, 3, "ldr < n");
  TG_ARG(n >= 1, 4, "n < 1");
  TG_ARG(k >= 1 && k <= n, 5, "k must be in [1, n]");
  TG_ARG(U, 6, "null U");
  TG_ARG(ldu >= n, 7, "ldu < n");
  hipStream_t st = (hipStream_t)stream;
  tg::Arena ar(ws, ws_bytes);
  double *S, *Y, *Bm, *A, *Tt, *Wb, *Rq;
  int *info;
  RefineWs rw{};
  urx_layout(ar, n, k, &S, &Y, &Bm, &A, &Tt, &Wb, &info, &Rq, &rw);
  TG_WS(ar);
  g_u_path = 0;
  const int mode = uqr_mode();
  TG_HIP(hipMemsetAsync(info, 0, sizeof(int), st));
  const bool two_chol = getenv("TG_URX_TWOCHOL") != nullptr;  // read per call (tests set it)
  if (!two_chol) {
    const int m = n - k;
    const dim3 gk(tg::cdiv(k, 256) < 16 ? tg::cdiv(k, 256) : 16, k);
    const bool small_m = urx_small_m(k, m);
    // C: k x m; the explicit form keeps its ld even so the DGEMMs that read
    // it stage 16-byte vectors
    const int ldc = small_m ? m : m + (m & 1);
    double *Yr = Y, *C = Bm, *ZT = S, *Nm = A;
    TG_HIP(hipMemsetAsync(Yr, 0, sizeof(double) * size_t(k) * k, st));
    hipLaunchKernelGGL(trinv_diag_kernel, dim3(tg::cdiv(k, NU)), dim3(256), 0, st, Rx, ldr, k, Yr,
                       k);
    TG_LAUNCHED();
    auto form_zt = [&](bool scratch_free) -> int {  // Z^T = R11 + R12 C^T
      TG_HIP(hipMemcpy2DAsync(ZT, sizeof(double) * k, Rx, sizeof(double) * ldr,
                              sizeof(double) * k, k, hipMemcpyDeviceToDevice, st));
      if (m <= 0) return 0;
      // the DGEMM stages 16-byte vectors only from 16-byte-aligned rows: with
      // an odd k R12's rows start mid-vector, so it is copied to an even-ld
      // buffer first (Y, when the caller says it is not live; C has an even
      // ld already)
      const int mp = m + (m & 1);
      const bool pad = scratch_free && ((k & 1) || (ldr & 1)) && mp <= k;
      if (pad) {
        double *R12p = Yr;
        TG_HIP(hipMemcpy2DAsync(R12p, sizeof(double) * mp, Rx + k, sizeof(double) * ldr,
                                sizeof(double) * m, k, hipMemcpyDeviceToDevice, st));
        TG_HIP(tg::dgemm(st, false, true, k, k, m, 1.0, R12p, mp, C, ldc, 1.0, ZT, k));
      } else {
        TG_HIP(tg::dgemm(st, false, true, k, k, m, 1.0, Rx + k, ldr, C, ldc, 1.0, ZT, k));
      }
      return 0;
    };
    if (small_m) {
      // C = R11^-1 R12 by block back substitution (no explicit inverse), and
      // N = Z Z^T = (R11 + R12 C^T)^T (R11 + R12 C^T) as
      //   R11^T R11 + V C^T + C V^T,  V = R11^T R12 + C (R12^T R12) / 2,
      // the first term a triangular SYRK (a third of the square's flops)
      if (m > 0) {
        TG_HIP(trinv_offdiag(st, Rx, ldr, Yr, k, k, Tt, TB));          // 256-block inverses
        if (const int e = trsm_upper_blocks(st, Rx, ldr, k, Rx + k, m, Yr, k, Nm, C, ldc)) return e;
      }
      if (mode != 2) {  // N is the Gram attempt's input only
        double *V = ZT, *G = Rq;  // k x m and m x m (ld m)
        if (m > 0) {
          TG_HIP(tg::dgemm(st, true, false, k, m, k, 1.0, Rx, ldr, Rx + k, ldr, 0.0, V, m));
          TG_HIP(tg::dgemm(st, true, false, m, m, k, 1.0, Rx + k, ldr, Rx + k, ldr, 0.0, G, m));
          TG_HIP(tg::dgemm(st, false, false, k, m, m, 0.5, C, m, G, m, 1.0, V, m));
        }
        TG_HIP(tg::dsyrk_tn_upper(st, k, 1.0, Rx, ldr, 0.0, Nm, k));     // R11^T R11
        if (m > 0) {
          TG_HIP(tg::dgemm(st, false, true, k, k, m, 1.0, ZT, m, C, m, 1.0, Nm, k));  // + V C^T
          TG_HIP(tg::dgemm(st, false, true, k, k, m, 1.0, C, m, ZT, m, 1.0, Nm, k));  // + C V^T
        }
      }
    } else {
      // C = R11^-1 R12 by block back substitution over 256-row blocks, as in
      // the small-m form (k^2 m flops, no k^3 / 3 inverse: n = 12,288 at
      // 3n/4 rank -14 ms); TG_URX_INV=1 (development switch, read per call)
      // keeps the explicit inverse and its triangular product
      const char *ui = getenv("TG_URX_INV");
      if (ui && ui[0] == '1') {
        TG_HIP(trinv_offdiag(st, Rx, ldr, Yr, k, k, Tt));             // Yr = R11^-1
        if (m > 0) TG_HIP(tg::dgemm_upper_a(st, k, m, k, 1.0, Yr, k, Rx + k, ldr, 0.0, C, ldc));
      } else if (m > 0) {
        TG_HIP(trinv_offdiag(st, Rx, ldr, Yr, k, k, Tt, TB));         // 256-block inverses
        if (const int e = trsm_upper_blocks(st, Rx, ldr, k, Rx + k, m, Yr, k, Nm, C, ldc)) return e;
      }
      if (const int e = urx_u11_from_c(st, Rx, ldr, n, k, C, ldc, U, ldu, Yr, ZT, Nm, Rq, Tt, Wb,
                                       info, rw))
        return e;
      if (m > 0)
        TG_HIP(tg::dgemm_upper_a(st, k, m, k, 1.0, U, ldu, C, ldc, 0.0, U + k, ldu));  // V^-1 C
      return 0;
    }
    CholStat h{};
    if (mode != 2) {
      hipLaunchKernelGGL(flip_both_kernel, gk, dim3(256), 0, st, Nm, k, Rq);  // N' = J N J
      TG_LAUNCHED();
      TG_HIP(chol_upper_rows(st, Rq, k, k, k, Wb, info));               // N' = R^T R
      hipLaunchKernelGGL(diag_range_kernel, dim3(1), dim3(256), 0, st, Rq, int64_t(k), k, rw.stats);
      TG_LAUNCHED();
      TG_HIP(read_stat(st, rw.stats, info, h));
    }
    if (mode == 2 || needs_refine(h)) {
      // R is the R factor of Yq = J Z^T J (Yq^T Yq = N'): CholeskyQR passes on
      // Yq, or its Householder QR
      double *Yq = Nm;
      if (mode != 2) TG_HIP(zero_lower(st, Rq, k, k));
      if (small_m) {  // ZT held V
        if (const int e = form_zt(false)) return e;
      }
      hipLaunchKernelGGL(flip_both_kernel, gk, dim3(256), 0, st, ZT, k, Yq);
      TG_LAUNCHED();
      const int e = refine_or_householder(st, Yq, k, Rq, rw, Wb, info, h, mode);
      if (e != 0) return e;
    }
    TG_HIP(trinv(st, Rq, k, k, Yr, Tt));                              // Yr = R^-1
    hipLaunchKernelGGL(flip_transpose_kernel, gk, dim3(256), 0, st, Yr, k, U, int64_t(ldu));
    TG_LAUNCHED();                                                    // U11 = V^-1 = J R^-T J
    if (m > 0)
      TG_HIP(tg::dgemm_upper_a(st, k, m, k, 1.0, U, ldu, C, ldc, 0.0, U + k, ldu));  // V^-1 C
    return 0;
  }
  CholStat h{};
  TG_HIP(tg::dsyrk_nt(st, k, n, 1.0, Rx, ldr, 0.0, S, k));        // S = R_x R_x^T
  TG_HIP(chol_upper_rows(st, S, k, k, k, Wb, info));                // S <- T, T^T T = S
  TG_HIP(read_stat(st, rw.stats, info, h));
  if (h.info > 0) {
    tg::set_error("U factor (two-Cholesky form): R_x R_x^T is not positive definite (%d pivots)",
                  h.info);
    return int(hipErrorUnknown);
  }
  TG_HIP(hipMemsetAsync(Y, 0, sizeof(double) * size_t(k) * k, st));
  hipLaunchKernelGGL(trinv_diag_kernel, dim3(tg::cdiv(k, NU)), dim3(256), 0, st, S, k, k, Y, k);
  TG_LAUNCHED();
  TG_HIP(trinv_offdiag(st, S, k, Y, k, k, Tt));                     // Y = T^-1
  TG_HIP(tg::dgemm(st, true, false, k, n, k, 1.0, Y, k, Rx, ldr, 0.0, Bm, n));  // T^-T R_x
  TG_HIP(tg::dgemm(st, false, false, k, n, k, 1.0, Y, k, Bm, n, 0.0, A, n));    // S^-1 R_x
  TG_HIP(tg::dgemm(st, true, false, k, n, k, 1.0, A, n, A, n, 0.0, U, ldu));    // G[:k, :]
  TG_HIP(chol_upper_rows(st, U, ldu, k, n, Wb, info));
  TG_HIP(zero_lower(st, U, ldu, k));
  TG_HIP(read_stat(st, rw.stats, info, h));
  if (h.info > 0) {
    tg::set_error("U factor (two-Cholesky form): Gram matrix not positive definite (%d pivots)",
                  h.info);
    return int(hipErrorUnknown);
  }
  return 0;
}

// ---------------------------------------------------------------------------
// The explicit-form U factor in column-sharded pieces (multi-GPU,
// gptq_svd_amd.dist.u_factor_rx_sharded): rank r computes C[:, c0:c1] =
// R11^-1 R12[:, c0:c1] (tg_urx_c), the ranks all-gather C, every rank forms
// U11 = V^-1 from the whole C (tg_urx_u11: Z, N, one k x k Cholesky, the
// triangular inverse -- replicated), then rank r its U12 columns V^-1 C[:,
// c0:c1] (tg_urx_u12) and the ranks all-gather U12.  Every C and U12 entry
// depends on its own column only (block back substitution, GEMMs with a
// fixed k order per entry), so the gathered U equals tg_u_factor_rx's
// explicit form bit for bit (tests/test_gpu_urx_sharded.py).  Workspace:
// tg_ufactor_rx_workspace_size(n, k).  The small-m form (m * 16 <= k, the
// near-full-rank layers) is not sharded: its C is a sliver.
// ---------------------------------------------------------------------------
extern "C" int tg_urx_c(void *stream, const double *Rx, int ldr, int n, int k, int c0, int c1,
                        double *C, int ldc, void *ws, size_t ws_bytes) {
  TG_ARG(Rx, 2, "null Rx");
  TG_ARG(ldr >= n, 3, "ldr < n");
  TG_ARG(k >= 1 && k <= n, 5, "k must be in [1, n]");
  TG_ARG(c0 >= 0 && c0 <= c1, 6, "c0 must be in [0, c1]");
  TG_ARG(c1 <= n - k, 7, "c1 > n - k");
  TG_ARG(C || c1 == c0, 8, "null C");
  TG_ARG(ldc >= c1 - c0, 9, "ldc < c1 - c0");
  hipStream_t st = (hipStream_t)stream;
  tg::Arena ar(ws, ws_bytes);
  double *S, *Y, *Bm, *A, *Tt, *Wb, *Rq;
  int *info;
  RefineWs rw{};
  urx_layout(ar, n, k, &S, &Y, &Bm, &A, &Tt, &Wb, &info, &Rq, &rw);
  TG_WS(ar);
  if (c1 == c0) return 0;
  if (const int e = urx_diag_inverses(st, Rx, ldr, k, Y, Tt)) return e;
  return trsm_upper_blocks(st, Rx, ldr, k, Rx + k + c0, c1 - c0, Y, k, A, C, ldc);
}

extern "C" int tg_urx_u11(void *stream, const double *Rx, int ldr, int n, int k, const double *C,
                          int ldc, double *U, int ldu, void *ws, size_t ws_bytes) {
  TG_ARG(Rx, 2, "null Rx");
  TG_ARG(ldr >= n, 3, "ldr < n");
  TG_ARG(k >= 1 && k <= n, 5, "k must be in [1, n]");
  TG_ARG(C || n == k, 6, "null C");
  TG_ARG(ldc >= n - k, 7, "ldc < n - k");
  TG_ARG(U, 8, "null U");
  TG_ARG(ldu >= n, 9, "ldu < n");
  hipStream_t st = (hipStream_t)stream;
  tg::Arena ar(ws, ws_bytes);
  double *S, *Y, *Bm, *A, *Tt, *Wb, *Rq;
  int *info;
  RefineWs rw{};
  urx_layout(ar, n, k, &S, &Y, &Bm, &A, &Tt, &Wb, &info, &Rq, &rw);
  TG_WS(ar);
  g_u_path = 0;
  TG_HIP(hipMemsetAsync(info, 0, sizeof(int), st));
  return urx_u11_from_c(st, Rx, ldr, n, k, C, ldc, U, ldu, Y, S, A, Rq, Tt, Wb, info, rw);
}

extern "C" int tg_urx_u12(void *stream, const double *U, int ldu, int k, const double *C, int ldc,
                          int ncols, double *out, int ldo) {
  TG_ARG(U, 2, "null U");
  TG_ARG(ldu >= k, 3, "ldu < k");
  TG_ARG(k >= 1, 4, "k < 1");
  TG_ARG(ncols >= 0, 7, "ncols < 0");
  TG_ARG(C || ncols == 0, 5, "null C");
  TG_ARG(out || ncols == 0, 8, "null out");
  TG_ARG(ldc >= ncols, 6, "ldc < ncols");
  TG_ARG(ldo >= ncols, 9, "ldo < ncols");
  if (ncols == 0) return 0;
  TG_HIP(tg::dgemm_upper_a((hipStream_t)stream, k, ncols, k, 1.0, U, ldu, C, ldc, 0.0, out, ldo));
  return 0;
}

namespace {
template <class A>
void hinv_layout(A &ar, int n, double **Aw, double **Yw, double **Tw, double **Wb, double **mean,
                 int **info) {
  const size_t h = size_t(NU) * ((tg::cdiv(n, NU) + 1) / 2);
  auto t = [&](auto *&dst, size_t cnt) {
    using T = std::remove_reference_t<decltype(*dst)>;
    dst = ar.template take<T>(cnt);
  };
  double *d0, *d1, *d2, *d3, *d4;
  int *i0;
  t(Aw ? *Aw : d0, size_t(n) * n);
  t(Yw ? *Yw : d1, size_t(n) * n);
  t(Tw ? *Tw : d2, h * h);
  t(Wb ? *Wb : d3, size_t(NU) * NU);
  t(mean ? *mean : d4, 1);
  t(info ? *info : i0, 16);
}
}  // namespace

extern "C" size_t tg_hinv_chol_workspace_size(int n) {
  tg::Sizer s;
  hinv_layout(s, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  return s.off + 256;
}

extern "C" int tg_hinv_chol(void *stream, const double *H, int n, int ldh, const int64_t *perm,
                            double damp_percent, int max_tries, double *R, int ldr,
                            int *tries_used, void *ws, size_t ws_bytes) {
  TG_ARG(H, 2, "null H");
  TG_ARG(n >= 1, 3, "n < 1");
  TG_ARG(ldh >= n, 4, "ldh < n");
  TG_ARG(max_tries >= 1, 7, "max_tries < 1");
  TG_ARG(R, 8, "null R");
  TG_ARG(ldr >= n, 9, "ldr < n");
  TG_ARG(tries_used, 10, "null tries_used");
  hipStream_t st = (hipStream_t)stream;
  tg::Arena ar(ws, ws_bytes);
  double *A, *Y, *T, *Wb, *mean;
  int *info;
  hinv_layout(ar, n, &A, &Y, &T, &Wb, &mean, &info);
  TG_WS(ar);
  const dim3 g2(tg::cdiv(n, 256) < 16 ? tg::cdiv(n, 256) : 16, n);
  hipLaunchKernelGGL(diag_mean_kernel, dim3(1), dim3(256), 0, st, H, int64_t(ldh), n, mean);
  TG_LAUNCHED();
  // damping ladder of gptq_utils.py:148-160: damp = 10^e * damp_percent
  double scale = 1.0;
  for (int e = 0; e < max_tries; ++e, scale *= 10.0) {
    hipLaunchKernelGGL(flip_damp_kernel, g2, dim3(256), 0, st, H, int64_t(ldh), n, perm,
                       scale * damp_percent, mean, A);
    TG_LAUNCHED();
    TG_HIP(hipMemsetAsync(info, 0, sizeof(int), st));
    TG_HIP(chol_upper_rows(st, A, n, n, n, Wb, info));
    int h_info = 0;
    TG_HIP(hipMemcpyAsync(&h_info, info, sizeof(int), hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    if (h_info != 0) continue;  // not positive definite at this damping: next rung
    TG_HIP(hipMemsetAsync(Y, 0, sizeof(double) * size_t(n) * n, st));
    hipLaunchKernelGGL(trinv_diag_kernel, dim3(tg::cdiv(n, NU)), dim3(256), 0, st, A, n, n, Y, n);
    TG_LAUNCHED();
    TG_HIP(trinv_offdiag(st, A, n, Y, n, n, T));
    hipLaunchKernelGGL(flip_transpose_kernel, g2, dim3(256), 0, st, Y, n, R, int64_t(ldr));
    TG_LAUNCHED();
    *tries_used = e;
    return 0;
  }
  // every rung failed: identity (the reference's intended fallback, :162-164)
  hipLaunchKernelGGL(identity_kernel, g2, dim3(256), 0, st, n, R, int64_t(ldr));
  TG_LAUNCHED();
  *tries_used = max_tries;
  return 0;
}
