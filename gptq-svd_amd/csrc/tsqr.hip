// Stage 1 of the two-stage eigensolver by the TSQR tree: the band reduction
// (sy2sb_tsqr) and its level-by-level back-transformation (sb_apply_q1_tsqr)
// for plans that are not `single` -- panels past the panel QR's row limit, or
// TG_SB_TSQR=1.  The production path is in band.hip.
//
//   panel P = A[r0:, p:p+32]  (m = n - r0 rows)
//   TSQR:  level 0 = Householder QR of each leaf of SB_C rows (one workgroup
//          per leaf, the leaf in LDS), level l+1 = QR of the stacked R factors
//          of level l, until one R remains.  Q = D_0 E_1 E_2 ... with D_0
//          block-diagonal over the leaves and E_l embedded on the rows that
//          carry level l's stacked R's.
//   A22 <- Q^T A22 Q, one level at a time, each as the compact-WY two-sided
//          update  X = A22 Y T,  W = X - 1/2 Y T^T Y^T X,  A22 -= Y W^T + W Y^T
//          with Y block-diagonal (chunked grouped GEMMs, gemm64.hip) and the
//          rank-64-per-tile symmetric update on lower tiles, mirrored, so A22
//          stays bitwise symmetric.
//   A[r0:, p:p+32] <- [R; 0]  (and its transpose).
//
// The reflectors (Y, T of every level of every panel) stay in the workspace
// for the back-transformation Z <- Q1 Z of the eigenvectors.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "band.h"
#include "gemm64.h"
#include "lanes.h"

namespace {

using tg::SB_B;
using tg::SB_C;

typedef double doublex4 __attribute__((ext_vector_type(4)));

// Row map of TSQR level lv: stacked row s of level lv -> row of level 0.
struct RowMap {
  int lv;
  int nc[tg::SB_LV];  // chunks of each level
  __device__ int fwd(int s) const { return tg::tsqr_row_fwd(lv, s); }
  __device__ int inv(int r) const {  // -1 if level-0 row r is not in the level's set
    for (int l = 1; l <= lv; ++l) {
      const int I = r / SB_C, o = r % SB_C;
      if (o >= SB_B || I >= nc[l - 1]) return -1;
      r = I * SB_B + o;
    }
    return r;
  }
};

__device__ inline double rcp_nr(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  return fma(fma(-x, r, 1.0), r, r);
}

// Reduce-scatter of the 32 products q_l = v0 r0[l] + v1 r1[l] over the wave,
// formed inside the first step: lane ends with the sum of column
// tg::lanes::rs_col(lane).  The two-array form of tg::lanes::reduce_scatter32,
// on the same swaps and DPP pairings (lanes.h).
__device__ inline double reduce_scatter32(const double (&r0)[32], const double (&r1)[32],
                                          double v0, double v1, int lane) {
  using namespace tg::lanes;
  auto qf = [&](int l) { return v0 * r0[l] + v1 * r1[l]; };
  double p[16];
  // lanes 0-31 keep column k, lanes 32-63 column k + 16
#pragma unroll
  for (int k = 0; k < 16; ++k) p[k] = rs_swap32(qf(k), qf(k + 16));
  // even 16-lane rows keep p[k], odd rows p[k + 8]
#pragma unroll
  for (int k = 0; k < 8; ++k) p[k] = rs_swap16(p[k], p[k + 8]);
  {
    const bool up = (lane & 8) != 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double recv = xdpp<DPP_MIRROR>(up ? p[k] : p[k + 4]);
      p[k] = (up ? p[k + 4] : p[k]) + recv;
    }
  }
  {
    const bool up = (lane & 4) != 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double recv = xdpp<DPP_HALF_MIRROR>(up ? p[k] : p[k + 2]);
      p[k] = (up ? p[k + 2] : p[k]) + recv;
    }
  }
  {
    const bool up = (lane & 2) != 0;
    const double recv = xdpp<DPP_XOR3>(up ? p[0] : p[1]);
    p[0] = (up ? p[1] : p[0]) + recv;
  }
  return p[0] + xdpp<DPP_XOR1>(p[0]);
}

// Householder QR of one leaf (chunk z of `m` rows, rows kb..ke of src, 32
// columns, row stride ld).  Thread t holds rows t and t + 256 in registers
// (rows >= h are zero, so every leaf runs exactly 32 steps: a zero
// subcolumn gives tau = 0).  Outputs (chunk layout, row-major, stride 32):
// Y rows kb..ke (unit lower trapezoid), YT = Y T, T[z] (dlarft
// forward/columnwise: H_0 H_1 ... = I - Y T Y^T), R[z] (32x32 upper).
// Per column one scalar and one 32-wide reduction; the latter gives both
// w = v^T P (trailing columns) and Y^T v (the new T column), and thread a of
// wave 0 extends row a of T in registers: T[a][j] = -tau_j sum_c T[a][c] q_c.
constexpr int QT = 256;
// STATS: per-phase s_memrealtime stamps (TG_QR_STATS); off in production, the
// stamps wait on lgkmcnt and lengthen the serial column chain.
template <bool STATS>
__global__ __launch_bounds__(QT) void tsqr_qr_kernel(const double *__restrict__ src, int64_t ld,
                                                     int c, int nc, int m,
                                                     double *__restrict__ Yo,
                                                     double *__restrict__ To,
                                                     double *__restrict__ Ro,
                                                     double *__restrict__ YTo,
                                                     unsigned long long *__restrict__ qst) {
  __shared__ double prow[SB_B];
  uint64_t ph[5] = {0, 0, 0, 0, 0};
  __shared__ double red[QT / 64][SB_B];
  __shared__ double qw[SB_B], taus[SB_B];
  __shared__ double Ts[SB_B][SB_B + 1];
  __shared__ double Gs[SB_B][SB_B + 1];
  const int z = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int kb = z * c, ke = (z == nc - 1) ? m : kb + c, h = ke - kb;
  double r0[SB_B], r1[SB_B];
  auto load_row = [&](int i, double(&r)[SB_B]) {
    if (i < h) {
      const double *p = src + int64_t(kb + i) * ld;
#pragma unroll
      for (int l = 0; l < SB_B; ++l) r[l] = p[l];
    } else {
#pragma unroll
      for (int l = 0; l < SB_B; ++l) r[l] = 0.0;
    }
  };
  load_row(tid, r0);
  load_row(tid + QT, r1);
  for (int idx = tid; idx < SB_B * (SB_B + 1); idx += QT) (&Ts[0][0])[idx] = 0.0;
  const int mycol = tg::lanes::rs_col(lane);
  // One reduction per column: with the raw column x as weights,
  // d_l = sum_{i>j} x_i P[i][l] gives both the squared norm (l = j) and,
  // since v = (x_i scal)_{i>j} with v_j = 1, every v^T P[:, l] =
  // P[j][l] + scal d_l (l > j: the update, l < j: the T recurrence input).
  auto step = [&](auto jc) {
    constexpr int j = decltype(jc)::value;
    const uint64_t p0 = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
    const double x0 = r0[j], x1 = r1[j];
    if (tid == j) {
#pragma unroll
      for (int l = 0; l < SB_B; ++l) prow[l] = r0[l];
    }
    const double d = reduce_scatter32(r0, r1, (tid > j) ? x0 : 0.0, x1, lane);
    const uint64_t p1 = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
    if ((lane & 1) == 0) red[wid][mycol] = d;
    __syncthreads();
    const uint64_t p2 = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
    const double s = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
    const double alpha = prow[j];
    double tau = 0.0, scal = 0.0, beta = alpha;
    if (s != 0.0) {
      beta = -copysign(sqrt(alpha * alpha + s), alpha);
      // reciprocals by v_rcp_f64 + two Newton steps (~1 ulp): the two IEEE
      // division sequences sit on the serial column chain
      tau = (beta - alpha) * rcp_nr(beta);
      scal = rcp_nr(alpha - beta);
    }
    const uint64_t p3 = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
    if (tid < SB_B) {
      const double dl = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
      const double a = prow[tid] + scal * dl;
      qw[tid] = a;
      Gs[tid][j] = tid < j ? a : 0.0;  // (Y^T v_j)_tid, the T recurrence input
    }
    if (tid == 0) taus[j] = tau;
    __syncthreads();
    const uint64_t p4 = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
    const double v0 = (tid > j) ? x0 * scal : (tid == j ? 1.0 : 0.0);
    const double v1 = x1 * scal;
    const double tv0 = tau * v0, tv1 = tau * v1;
#pragma unroll
    for (int l = j + 1; l < SB_B; ++l) {
      const double w = qw[l];
      r0[l] -= tv0 * w;
      r1[l] -= tv1 * w;
    }
    r0[j] = (tid > j) ? v0 : (tid == j ? beta : x0);
    r1[j] = v1;
    const uint64_t p5 = STATS ? __builtin_amdgcn_s_memrealtime() : 0;
    if constexpr (STATS) {
      ph[0] += p1 - p0; ph[1] += p2 - p1; ph[2] += p3 - p2; ph[3] += p4 - p3; ph[4] += p5 - p4;
    }
  };
  [&]<int... J>(std::integer_sequence<int, J...>) {
    (step(std::integral_constant<int, J>{}), ...);
  }(std::make_integer_sequence<int, SB_B>{});
  if (STATS && qst && tid == 0) {
    for (int k = 0; k < 5; ++k) atomicAdd(qst + k, (unsigned long long)ph[k]);
    atomicAdd(qst + 5, 1ull);
  }
  // T (dlarft, forward columnwise): row a is independent of the other rows:
  // T[a][j] = -tau_j sum_{c<j} T[a][c] G[c][j], T[a][a] = tau_a, T[a][c<a] = 0.
  __syncthreads();
  if (tid < SB_B) {
    double trow[SB_B];
#pragma unroll
    for (int c2 = 0; c2 < SB_B; ++c2) trow[c2] = 0.0;
#pragma unroll
    for (int j = 0; j < SB_B; ++j) {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
      for (int c2 = 0; c2 < j; c2 += 4) {
        a0 += trow[c2] * Gs[c2][j];
        if (c2 + 1 < j) a1 += trow[c2 + 1] * Gs[c2 + 1][j];
        if (c2 + 2 < j) a2 += trow[c2 + 2] * Gs[c2 + 2][j];
        if (c2 + 3 < j) a3 += trow[c2 + 3] * Gs[c2 + 3][j];
      }
      const double tj = taus[j];
      trow[j] = (tid < j) ? -tj * ((a0 + a1) + (a2 + a3)) : (tid == j ? tj : 0.0);
    }
#pragma unroll
    for (int c2 = 0; c2 < SB_B; ++c2) Ts[tid][c2] = trow[c2];
  }
  if (tid < SB_B) {
    double *ro = Ro + size_t(z) * SB_B * SB_B + tid * SB_B;
#pragma unroll
    for (int l = 0; l < SB_B; ++l) ro[l] = (l >= tid) ? r0[l] : 0.0;
  }
  __syncthreads();
  auto emit = [&](int i, double(&r)[SB_B]) {
    if (i >= h) return;
#pragma unroll
    for (int l = 0; l < SB_B; ++l) r[l] = (i == l) ? 1.0 : (i > l ? r[l] : 0.0);  // Y row
    double *yo = Yo + int64_t(kb + i) * SB_B;
    double *yt = YTo + int64_t(kb + i) * SB_B;
#pragma unroll
    for (int l = 0; l < SB_B; ++l) yo[l] = r[l];
#pragma unroll
    for (int l = 0; l < SB_B; ++l) {
      double a = 0.0;
#pragma unroll
      for (int a2 = 0; a2 <= l; ++a2) a += r[a2] * Ts[a2][l];
      yt[l] = a;
    }
  };
  emit(tid, r0);
  emit(tid + QT, r1);
  for (int idx = tid; idx < SB_B * SB_B; idx += QT)
    To[size_t(z) * SB_B * SB_B + idx] = Ts[idx >> 5][idx & 31];
}

hipError_t launch_qr(hipStream_t st, const double *src, int64_t ld, int nc, int m, double *Y,
                     double *T, double *R, double *YT) {
  const int hmax = (nc == 1) ? m : std::max(SB_C, m - (nc - 1) * SB_C);
  if (hmax > 2 * QT) return hipErrorInvalidValue;
  // Householder QR of the nc leaves: ~2 h b^2 flops per leaf
  auto tok = tg::prof_begin(st, tg::PROF_TSQR, 16.0 * m * SB_B, 2.0 * m * SB_B * SB_B);
  static unsigned long long *qst = nullptr;
  static bool want = getenv("TG_QR_STATS") != nullptr;
  if (want && !qst) {
    (void)hipMalloc(&qst, 8 * sizeof(unsigned long long));
    (void)hipMemset(qst, 0, 8 * sizeof(unsigned long long));
    atexit([] {
      unsigned long long h[8];
      (void)hipMemcpy(h, qst, sizeof(h), hipMemcpyDeviceToHost);
      fprintf(stderr, "qr per column (us): rs %.2f  red+bar %.2f  scal %.2f  qv+bar %.2f  upd %.2f (WGs %llu)\n",
              h[0] / 100.0 / h[5] / 32, h[1] / 100.0 / h[5] / 32, h[2] / 100.0 / h[5] / 32,
              h[3] / 100.0 / h[5] / 32, h[4] / 100.0 / h[5] / 32, h[5]);
    });
  }
  if (qst)
    hipLaunchKernelGGL(tsqr_qr_kernel<true>, dim3(nc), dim3(QT), 0, st, src, ld, SB_C, nc, m, Y, T,
                       R, YT, qst);
  else
    hipLaunchKernelGGL(tsqr_qr_kernel<false>, dim3(nc), dim3(QT), 0, st, src, ld, SB_C, nc, m, Y, T,
                       R, YT, nullptr);
  tg::prof_end(st, tok);
  return hipGetLastError();
}

// Per (column block J of 32, chunk I): P = Y_I^T Z[chunk rows, J cols]
// (32 x 32) on FP64 MFMA, then
//   MODE 0: M[I-block rows, J-block cols] = T_I^T P            (two-sided update)
//   MODE 1: Z[chunk rows, J cols] -= Y_I (T_I P)                (back-transform Q Z)
// 8 waves, wave w owns chunk rows 64w..64w+63 (chunks hold < 512 rows) as
// eight 16x16 C-layout fragments; since the f64 MFMA C/D layout (lane l,
// reg q -> row (l>>4)+4q, col l&15) equals the B-operand layout for four
// consecutive K-steps, the same registers are the B operand of P = Y^T Z and
// the accumulator of Z -= Y (T P).  GATHER: stacked row s lives at Z row
// map(s) (TSQR levels >= 1).
template <int MODE, bool GATHER>
__global__ __launch_bounds__(512) void ytz_kernel(const double *__restrict__ Y,
                                                  const double *__restrict__ T,
                                                  double *__restrict__ Z, int64_t ldz, int ncols,
                                                  int c, int nc, int rows, RowMap mp,
                                                  double *__restrict__ M, int64_t ldm) {
  __shared__ double red[8][SB_B][SB_B + 1];
  __shared__ double Ps[SB_B][SB_B + 1];
  __shared__ double Ms[SB_B][SB_B + 1];
  const int J = blockIdx.x, I = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int kb = I * c, ke = (I == nc - 1) ? rows : kb + c;
  const int h = ke - kb;
  const int c0 = J * SB_B;
  const int lr = lane >> 4, lc = lane & 15;
  doublex4 F[4][2];
  // load the wave's 64 x 32 slab of Z (zeros outside the chunk / columns)
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int rl = wid * 64 + rb * 16 + lr + 4 * q;
      const int rc = min(rl, h - 1);
      const int zr = GATHER ? mp.fwd(kb + rc) : kb + rc;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
        F[rb][cb][q] = Z[int64_t(zr) * ldz + min(c0 + cb * 16 + lc, ncols - 1)];
    }
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int rl = wid * 64 + rb * 16 + lr + 4 * q;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
        F[rb][cb][q] = (rl < h && c0 + cb * 16 + lc < ncols) ? F[rb][cb][q] : 0.0;
    }
  // P_w = Y_w^T Z_w
  doublex4 Pa[2][2];
#pragma unroll
  for (int ia = 0; ia < 2; ++ia)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) Pa[ia][cb] = doublex4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int rl = wid * 64 + rb * 16 + 4 * q + lr;
      double ya[2];
#pragma unroll
      for (int ia = 0; ia < 2; ++ia)
        ya[ia] = Y[int64_t(kb + min(rl, h - 1)) * SB_B + ia * 16 + lc];
#pragma unroll
      for (int ia = 0; ia < 2; ++ia) ya[ia] = rl < h ? ya[ia] : 0.0;
#pragma unroll
      for (int ia = 0; ia < 2; ++ia)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
          Pa[ia][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya[ia], F[rb][cb][q], Pa[ia][cb], 0, 0, 0);
    }
#pragma unroll
  for (int ia = 0; ia < 2; ++ia)
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[wid][ia * 16 + lr + 4 * q][cb * 16 + lc] = Pa[ia][cb][q];
  __syncthreads();
  for (int idx = tid; idx < SB_B * SB_B; idx += 512) {
    const int a = idx >> 5, cc = idx & 31;
    double v = 0.0;
#pragma unroll
    for (int w = 0; w < 8; ++w) v += red[w][a][cc];
    Ps[a][cc] = v;
  }
  __syncthreads();
  for (int idx = tid; idx < SB_B * SB_B; idx += 512)
    Ms[idx >> 5][idx & 31] = T[size_t(I) * SB_B * SB_B + idx];
  __syncthreads();
  double mval[2];
  for (int idx = tid, t = 0; idx < SB_B * SB_B; idx += 512, ++t) {
    const int a = idx >> 5, cc = idx & 31;
    double v = 0.0;
    if (MODE == 0) {
      for (int e = 0; e <= a; ++e) v += Ms[e][a] * Ps[e][cc];
      if (c0 + cc < ldm) M[int64_t(I * SB_B + a) * ldm + c0 + cc] = v;
    } else {
      for (int e = a; e < SB_B; ++e) v += Ms[a][e] * Ps[e][cc];
      mval[t] = v;
    }
  }
  if (MODE == 0) return;
  __syncthreads();  // T no longer read: Ms <- T P
  for (int idx = tid, t = 0; idx < SB_B * SB_B; idx += 512, ++t) Ms[idx >> 5][idx & 31] = mval[t];
  __syncthreads();
  // Z_w -= Y_w Ms
#pragma unroll
  for (int k0 = 0; k0 < SB_B; k0 += 4) {
    double bm[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) bm[cb] = Ms[k0 + lr][cb * 16 + lc];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      const int rl = wid * 64 + rb * 16 + lc;
      const double yl = Y[int64_t(kb + min(rl, h - 1)) * SB_B + k0 + lr];
      const double ya = rl < h ? -yl : 0.0;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
        F[rb][cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(ya, bm[cb], F[rb][cb], 0, 0, 0);
    }
  }
#pragma unroll
  for (int rb = 0; rb < 4; ++rb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int rl = wid * 64 + rb * 16 + lr + 4 * q;
      if (rl >= h) continue;
      const int zr = GATHER ? mp.fwd(kb + rl) : kb + rl;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const int col = c0 + cb * 16 + lc;
        if (col < ncols) Z[int64_t(zr) * ldz + col] = F[rb][cb][q];
      }
    }
}

// A22 -= Yd X^T + X Yd^T - Yd S Yd^T,  S = (M + M^T)/2  (== Yd W^T + W Yd^T
// with W = X - Yd M / 2).  Yd block-diagonal over chunks of c rows:
//   (Yd X^T)[r][c'] = sum_l Y[r][l] X[c'][I(r)*32 + l]
//   (X Yd^T)[r][c'] = sum_l X[r][J(c')*32 + l] Y[c'][l]
//   (Yd S Yd^T)[r][c'] = (Y[r] S_{I(r)J(c')}) . Y[c']
// 64x64 lower tiles (c is a multiple of 64: a tile lies in one chunk),
// K = 96 in three segments, mirrored: A22 stays bitwise symmetric.
constexpr int S2T = 64, S2K = 16, S2P = 4;
__global__ __launch_bounds__(256) void syr2k_bs_kernel(double *__restrict__ A, int64_t lda, int m,
                                                       int c, int nc,
                                                       const double *__restrict__ Y,
                                                       const double *__restrict__ X,
                                                       int64_t ldx,
                                                       const double *__restrict__ M,
                                                       int64_t ldm) {
  // one LDS block: As, Bs, YS during the K loop, then the 64 x 65 tile for the
  // coalesced mirror stores
  constexpr int SMN = (2 * S2K + SB_B) * (S2T + S2P);
  static_assert(SMN >= S2T * (S2T + 1), "mirror tile must fit");
  __shared__ double sm[SMN];
  double(*As)[S2T + S2P] = reinterpret_cast<double(*)[S2T + S2P]>(sm);
  double(*Bs)[S2T + S2P] = reinterpret_cast<double(*)[S2T + S2P]>(sm + S2K * (S2T + S2P));
  double(*YS)[S2T + S2P] = reinterpret_cast<double(*)[S2T + S2P]>(sm + 2 * S2K * (S2T + S2P));  // -(Y_rows S_IJ)^T, k-major
  __shared__ double Ss[SB_B][SB_B + 1];
  const int b = blockIdx.x;
  int I = int((sqrt(8.0 * b + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= b) ++I;
  while (I * (I + 1) / 2 > b) --I;
  const int J = b - I * (I + 1) / 2;
  const int tm = I * S2T, tn = J * S2T;
  const int ci = min(tm / c, nc - 1), cj = min(tn / c, nc - 1);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  // the tile's old values first (clamped addresses): their HBM latency
  // overlaps the S / YS set-up and the K loop instead of following it
  double old[2][2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = min(tm + wm * 32 + i * 16 + (lane >> 4) + 4 * r, m - 1);
        const int gj = min(tn + wn * 32 + j * 16 + (lane & 15), m - 1);
        old[i][j][r] = A[int64_t(gi) * lda + gj];
      }
  // S_IJ and YS = -(Y_rows S_IJ)
  for (int idx = tid; idx < SB_B * SB_B; idx += 256) {
    const int x = idx >> 5, y = idx & 31;
    Ss[x][y] = 0.5 * (M[int64_t(ci * SB_B + x) * ldm + cj * SB_B + y] +
                      M[int64_t(cj * SB_B + y) * ldm + ci * SB_B + x]);
  }
  __syncthreads();
  {
    const int i = tid >> 2, b0 = (tid & 3) * 8;  // row i, columns b0..b0+7
    const int gr = tm + i;
    double yr[SB_B];
#pragma unroll
    for (int l = 0; l < SB_B; ++l) yr[l] = gr < m ? Y[int64_t(gr) * SB_B + l] : 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      double v = 0.0;
#pragma unroll
      for (int l = 0; l < SB_B; ++l) v += yr[l] * Ss[l][b0 + q];
      YS[b0 + q][i] = -v;
    }
  }
  doublex4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = doublex4{0.0, 0.0, 0.0, 0.0};
  const int sr = tid >> 2, sk = (tid & 3) * 4;
  for (int k0 = 0; k0 < 3 * SB_B; k0 += S2K) {
    const int seg = k0 / SB_B;
    const int kl = (k0 & 31) + sk;
    double va[4], vb[4];
    {
      const int gr = tm + sr, grc = min(gr, m - 1);
      const double *src = seg ? X + int64_t(grc) * ldx + cj * SB_B + kl : Y + int64_t(grc) * SB_B + kl;
#pragma unroll
      for (int t = 0; t < 4; ++t) va[t] = src[t];
    }
    {
      const int gr = tn + sr, grc = min(gr, m - 1);
      const double *src = seg == 0 ? X + int64_t(grc) * ldx + ci * SB_B + kl : Y + int64_t(grc) * SB_B + kl;
#pragma unroll
      for (int t = 0; t < 4; ++t) vb[t] = src[t];
    }
    if (seg < 2) {
#pragma unroll
      for (int t = 0; t < 4; ++t) As[sk + t][sr] = tm + sr < m ? va[t] : 0.0;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) Bs[sk + t][sr] = tn + sr < m ? vb[t] : 0.0;
    __syncthreads();
    double(*Ap)[S2T + S2P] = seg < 2 ? As : YS + (k0 & 31);
#pragma unroll
    for (int kq = 0; kq < S2K; kq += 4) {
      double af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = Ap[kq + (lane >> 4)][wm * 32 + i * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = Bs[kq + (lane >> 4)][wn * 32 + j * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  // the lower tile written and, for an off-diagonal tile, its transpose
  // written row-contiguous from LDS
  double(*Tt)[S2T + 1] = reinterpret_cast<double(*)[S2T + 1]>(sm);  // K loop done (barrier)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int li = wm * 32 + i * 16 + (lane >> 4) + 4 * r, lj = wn * 32 + j * 16 + (lane & 15);
        const int gi = tm + li, gj = tn + lj;
        if (gi < m && gj < m && gi >= gj) {
          const double v = old[i][j][r] - acc[i][j][r];
          A[int64_t(gi) * lda + gj] = v;
          if (tm != tn) Tt[li][lj] = v;
          else if (gi != gj) A[int64_t(gj) * lda + gi] = v;
        }
      }
  if (tm != tn) {
    __syncthreads();
    for (int idx = tid; idx < S2T * S2T; idx += 256) {
      const int lc = idx >> 6, lr = idx & 63;  // row tn + lc, column tm + lr
      if (tn + lc < m && tm + lr < m) A[int64_t(tn + lc) * lda + tm + lr] = Tt[lr][lc];
    }
  }
}

// Both passes of sym_scatter_kernel in one launch: blockIdx.z = pass, each
// with its own (x, y) extent; the passes write disjoint entries.
__global__ void sym_scatter2_kernel(double *__restrict__ A, int64_t lda, int m, int nS, RowMap mp,
                                    const double *__restrict__ U, int gx0, int gx1, int gy1) {
  if (blockIdx.z == 0) {
    const int s = blockIdx.y;
    if (s >= nS || int(blockIdx.x) >= gx0) return;
    const int r = mp.fwd(s);
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < m; c += gx0 * blockDim.x) {
      const int t = mp.inv(c);
      double v = U[int64_t(s) * m + c];
      if (t >= 0) v = v + U[int64_t(t) * m + r];
      A[int64_t(r) * lda + c] -= v;
    }
  } else {
    if (int(blockIdx.x) >= gx1 || int(blockIdx.y) >= gy1) return;
    const int r = blockIdx.x * 64 + (threadIdx.x & 63);
    if (r >= m || mp.inv(r) >= 0) return;
    for (int t = blockIdx.y * 4 + (threadIdx.x >> 6); t < nS; t += gy1 * 4)
      A[int64_t(r) * lda + mp.fwd(t)] -= U[int64_t(t) * m + r];
  }
}

// X[S_s, :] -= 1/2 sum_a Y[s][a] M[z(s) * 32 + a][:]  (z(s) = chunk of level
// row s), in place through the row map: the level >= 1 W = X - Yd M / 2.
__global__ void xs_update_kernel(double *__restrict__ X, int w, int rows, int nc, RowMap mp,
                                 const double *__restrict__ Y, const double *__restrict__ M) {
  const int s = blockIdx.y, col = blockIdx.x * 64 + threadIdx.x;
  if (col >= w) return;
  const int z = min(s / SB_C, nc - 1);
  const double *yr = Y + int64_t(s) * SB_B;
  const double *mc = M + int64_t(z) * SB_B * w + col;
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < SB_B; ++a) acc += yr[a] * mc[int64_t(a) * w];
  X[int64_t(mp.fwd(s)) * w + col] += -0.5 * acc;
}

// dst[s][:] = src[map(s)][:]
__global__ void gather_rows_kernel(const double *__restrict__ src, int64_t lds, int ncols, int nrows,
                                   RowMap mp, double *__restrict__ dst) {
  const int s = blockIdx.y;
  const int r = mp.fwd(s);
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncols; c += gridDim.x * blockDim.x)
    dst[int64_t(s) * ncols + c] = src[int64_t(r) * lds + c];
}

// dst[map(s)][:] = src[s][:]
__global__ void scatter_rows_kernel(const double *__restrict__ src, int ncols, int nrows, RowMap mp,
                                    double *__restrict__ dst, int64_t ldd) {
  const int s = blockIdx.y;
  const int r = mp.fwd(s);
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < ncols; c += gridDim.x * blockDim.x)
    dst[int64_t(r) * ldd + c] = src[int64_t(s) * ncols + c];
}

// A22 -= Ye U^T... in scattered form: U (nS x m) = Y_l W^T.
//   z = 0: rows map(s): A[map(s)][c] -= U[s][c] + (c in set ? U[t(c)][map(s)] : 0)
//   z = 1: rows r not in set, columns map(t): A[r][map(t)] -= U[t][r]
__global__ void sym_scatter_kernel(double *__restrict__ A, int64_t lda, int m, int nS, RowMap mp,
                                   const double *__restrict__ U, int pass) {
  if (pass == 0) {
    const int s = blockIdx.y;
    if (s >= nS) return;
    const int r = mp.fwd(s);
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < m; c += gridDim.x * blockDim.x) {
      const int t = mp.inv(c);
      double v = U[int64_t(s) * m + c];
      if (t >= 0) v = v + U[int64_t(t) * m + r];
      A[int64_t(r) * lda + c] -= v;
    }
  } else {
    // rows r = blockIdx.x * 64 + (tid & 63), columns t = blockIdx.y*4 + (tid >> 6) ...
    const int r = blockIdx.x * 64 + (threadIdx.x & 63);
    if (r >= m || mp.inv(r) >= 0) return;
    for (int t = blockIdx.y * 4 + (threadIdx.x >> 6); t < nS; t += gridDim.y * 4)
      A[int64_t(r) * lda + mp.fwd(t)] -= U[int64_t(t) * m + r];
  }
}

// A[r0+i][p+l] = [R; 0] and the transpose (i < m, l < 32).
__global__ void write_panel_kernel(double *__restrict__ A, int64_t lda, int p, int r0, int m,
                                   const double *__restrict__ R) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= m * SB_B) return;
  const int i = idx >> 5, l = idx & 31;
  const double v = (i < SB_B) ? R[i * SB_B + l] : 0.0;
  A[int64_t(r0 + i) * lda + p + l] = v;
  A[int64_t(p + l) * lda + r0 + i] = v;
}

}  // namespace

namespace tg {

hipError_t sy2sb_tsqr(hipStream_t st, double *A, int lda, const SbPlan &pl, const SbBufs &b) {
  SideStream *ss = nullptr;
  TG_CHK(side_stream(ss));
  int pi = 0;
  for (const SbPanel &P : pl.panels) {
    const int m = P.m, r0 = P.r0;
    double *A22 = A + int64_t(r0) * lda + r0;
    RowMap mp{};
    for (int l = 0; l < P.nl; ++l) mp.nc[l] = P.L[l].nc;
    // level-0 QR on the main stream; levels >= 1 (QR of the stacked R's) on
    // the side stream, overlapping level 0's two-sided update.
    TG_CHK(launch_qr(st, A + int64_t(r0) * lda + P.p, lda, P.L[0].nc, m, b.Y + P.L[0].yoff,
                     b.T + P.L[0].toff, b.R[0], b.YT));
    const int ph = pi & 1;
    if (P.nl > 1) {
      TG_CHK(hipEventRecord(ss->ev0[ph], st));
      TG_CHK(hipStreamWaitEvent(ss->s, ss->ev0[ph], 0));
      for (int l = 1; l < P.nl; ++l) {
        const SbLevel &L = P.L[l];
        TG_CHK(launch_qr(ss->s, b.R[(l - 1) & 1], SB_B, L.nc, L.rows, b.Y + L.yoff, b.T + L.toff,
                         b.R[l & 1], b.YTl[l]));
      }
      TG_CHK(hipEventRecord(ss->ev1[ph], ss->s));
      // R (in R[1] when nl is even) -> the panel's band block, off the main
      // stream's critical path: it writes A outside every later A22 and
      // outside the next panels' columns; joined after the last panel
      if (((P.nl - 1) & 1) == 1) {
        hipLaunchKernelGGL(write_panel_kernel, dim3(cdiv(m * SB_B, 256)), dim3(256), 0, ss->s, A,
                           int64_t(lda), P.p, r0, m, b.R[1]);
        TG_CHK(hipGetLastError());
      }
    }
    for (int l = 0; l < P.nl; ++l) {
      const SbLevel &L = P.L[l];
      double *Yl = b.Y + L.yoff, *Tl = b.T + L.toff;
      const int nc = L.nc, rows = L.rows, w = nc * SB_B;
      mp.lv = l;
      if (l == 0) {
        // X = A22 blockdiag(YT)   (m x w)
        ChunkSpec cx{SB_C, nc, m, 1, 0, SB_B, 0, 0, SB_B, m, SB_B, -1};
        TG_CHK(dgemm_chunked(st, false, false, cx, 1.0, A22, lda, b.YT, SB_B, 0.0, b.X, w));
        // M = Td^T Yd^T X  (w x w)
        hipLaunchKernelGGL((ytz_kernel<0, false>), dim3(nc, nc), dim3(512), 0, st, Yl, Tl, b.X,
                           int64_t(w), w, SB_C, nc, m, mp, b.M, int64_t(w));
        TG_CHK(hipGetLastError());
        const int nt = cdiv(m, S2T);
        // HBM: lower tiles of A22 read, both triangles written (1.5 m^2 doubles)
        auto tok = prof_begin(st, PROF_SBUPD, 12.0 * double(m) * m, 96.0 * double(m) * m);
        hipLaunchKernelGGL(syr2k_bs_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, st, A22,
                           int64_t(lda), m, SB_C, nc, Yl, b.X, int64_t(w), b.M, int64_t(w));
        prof_end(st, tok);
        TG_CHK(hipGetLastError());
        if (P.nl > 1) TG_CHK(hipStreamWaitEvent(st, ss->ev1[ph], 0));
      } else {
        double *YTl = b.YTl[l];
        // X = A22[S, :]^T blockdiag(YT)   (m x w)
        if (nc == 1) {
          // one chunk (w = 32): the rows S are 32-row blocks of A22 at a
          // fixed stride, so X = sum_z A22[block z, :]^T YT[32z : 32z + 32, :]
          // is one chunked GEMM straight from A22 (no gather; nz x 64 output
          // tiles instead of m/64) and a sum of the nz partials (scratch: U,
          // which this level fills only later; nz * 32 * m <= ncmax * 32 * n)
          int stride = SB_C;
          for (int q = 1; q < l; ++q) stride *= SB_C / SB_B;
          const int nz = rows / SB_B;
          ChunkSpec cz{SB_B, nz, rows, int64_t(stride / SB_B) * lda, 0, SB_B, 0, 0,
                       int64_t(m) * SB_B, m, SB_B, SB_B};
          TG_CHK(dgemm_chunked(st, true, false, cz, 1.0, A22, lda, YTl, SB_B, 0.0, b.U, SB_B));
          TG_CHK(sum_partials(st, b.U, nz, m, SB_B, 1.0, 0.0, b.X, w));
        } else {
          // Gr = A22[S, :]  (rows x m)
          hipLaunchKernelGGL(gather_rows_kernel, dim3(cdiv(m, 256), rows), dim3(256), 0, st, A22,
                             int64_t(lda), m, rows, mp, b.Gr);
          TG_CHK(hipGetLastError());
          ChunkSpec cx{SB_C, nc, rows, m, 0, SB_B, 0, 0, SB_B, m, SB_B, -1};
          TG_CHK(dgemm_chunked(st, true, false, cx, 1.0, b.Gr, m, YTl, SB_B, 0.0, b.X, w));
        }
        // M = T^T Y^T X[S, :]  (the rows S of X read through the row map)
        hipLaunchKernelGGL((ytz_kernel<0, true>), dim3(nc, nc), dim3(512), 0, st, Yl, Tl, b.X,
                           int64_t(w), w, SB_C, nc, rows, mp, b.M, int64_t(w));
        TG_CHK(hipGetLastError());
        // W = X - 1/2 Yd M on the rows S, in place
        hipLaunchKernelGGL(xs_update_kernel, dim3(cdiv(w, 64), rows), dim3(64), 0, st, b.X, w,
                           rows, nc, mp, Yl, b.M);
        TG_CHK(hipGetLastError());
        // U = Y_l W^T  (rows x m)
        ChunkSpec cu{SB_C, nc, rows, SB_B, 0, 0, SB_B, m, 0, -1, m, SB_B};
        TG_CHK(dgemm_chunked(st, false, true, cu, 1.0, Yl, SB_B, b.X, w, 0.0, b.U, m));
        // A22[S, :] and A22[:, S] -= U, U^T in one launch (disjoint entries)
        {
          const int gx0 = cdiv(m, 256), gx1 = cdiv(m, 64), gy1 = std::min(64, cdiv(rows, 4));
          hipLaunchKernelGGL(sym_scatter2_kernel, dim3(std::max(gx0, gx1), std::max(rows, gy1), 2),
                             dim3(256), 0, st, A22, int64_t(lda), m, rows, mp, b.U, gx0, gx1, gy1);
          TG_CHK(hipGetLastError());
        }
      }
    }
    if (((P.nl - 1) & 1) == 0) {
      hipLaunchKernelGGL(write_panel_kernel, dim3(cdiv(m * SB_B, 256)), dim3(256), 0, st, A,
                         int64_t(lda), P.p, r0, m, b.R[(P.nl - 1) & 1]);
      TG_CHK(hipGetLastError());
    }
    ++pi;
  }
  TG_CHK(hipEventRecord(ss->evj, ss->s));  // side-stream panel writes done
  TG_CHK(hipStreamWaitEvent(st, ss->evj, 0));
  return hipSuccess;
}

hipError_t sb_apply_q1_tsqr(hipStream_t st, double *Z, int k, const SbPlan &pl, const SbBufs &b) {
  for (auto it = pl.panels.rbegin(); it != pl.panels.rend(); ++it) {
    const SbPanel &P = *it;
    double *Zs = Z + int64_t(P.r0) * k;
    RowMap mp{};
    for (int l = 0; l < P.nl; ++l) mp.nc[l] = P.L[l].nc;
    for (int l = P.nl - 1; l >= 0; --l) {  // Q = D_0 E_1 E_2 ...: top level first
      const SbLevel &L = P.L[l];
      mp.lv = l;
      // HBM: read + write of the level's rows of Z
      auto tok = prof_begin(st, PROF_Q1, 16.0 * double(L.rows) * k, 4.0 * double(L.rows) * SB_B * k);
      if (l > 0)
        hipLaunchKernelGGL((ytz_kernel<1, true>), dim3(cdiv(k, SB_B), L.nc), dim3(512), 0, st,
                           b.Y + L.yoff, b.T + L.toff, Zs, int64_t(k), k, SB_C, L.nc, L.rows, mp,
                           nullptr, int64_t(0));
      else
        hipLaunchKernelGGL((ytz_kernel<1, false>), dim3(cdiv(k, SB_B), L.nc), dim3(512), 0, st,
                           b.Y + L.yoff, b.T + L.toff, Zs, int64_t(k), k, SB_C, L.nc, L.rows, mp,
                           nullptr, int64_t(0));
      prof_end(st, tok);
      TG_CHK(hipGetLastError());
    }
  }
  return hipSuccess;
}

}  // namespace tg
