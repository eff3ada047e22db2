// Stage 1 of the two-stage eigensolver, production path (band.hip
// sy2sb_single): what follows a panel's X / M launch -- W from X and M, the
// update of a pair partner's columns, and the trailing update A22 -= Y W^T +
// W Y^T of one panel (rank 64) or of a pair (rank 128).  Each kernel behind a
// launch_* function declared in band.h.
#include <algorithm>
#include <cmath>

#include "band.h"

namespace {

using tg::SB_B;

typedef double doublex4 __attribute__((ext_vector_type(4)));

// Single-level panels: W = X - 1/2 Y M in place over X (m x 32 each, M 32 x
// 32), so the trailing update is the rank-64 A22 -= Y W^T + W Y^T (K = 64
// instead of the TSQR path's K = 96 form, which folds Y S Y^T into the tiles).
// One workgroup per 16 rows (m / 16 workgroups: the latency of one row's
// loads, not a queue of rows, sets the time): M in LDS, the thread's Y row
// and X pair straight from L2, two outputs per thread.
constexpr int WU_R = 16;
__global__ __launch_bounds__(256) void w_update_kernel(const double *__restrict__ Y,
                                                       double *__restrict__ X, int m,
                                                       const double *__restrict__ M) {
  __shared__ double2 Ms[SB_B][SB_B / 2];
  const int tid = threadIdx.x;
  const int r = blockIdx.x * WU_R + (tid >> 4), c2 = tid & 15;  // row r, columns 2c2, 2c2 + 1
  const int rc = min(r, m - 1);
  double2 y[SB_B / 2];
#pragma unroll
  for (int h = 0; h < SB_B / 2; ++h) y[h] = reinterpret_cast<const double2 *>(Y + int64_t(rc) * SB_B)[h];
  const double2 x = reinterpret_cast<const double2 *>(X + int64_t(rc) * SB_B)[c2];
  for (int e = tid; e < SB_B * SB_B / 2; e += 256)
    Ms[e >> 4][e & 15] = reinterpret_cast<const double2 *>(M)[e];
  __syncthreads();
  double v0 = 0.0, v1 = 0.0;
#pragma unroll
  for (int h = 0; h < SB_B / 2; ++h) {
    const double2 a = Ms[2 * h][c2], b = Ms[2 * h + 1][c2];
    v0 = fma(y[h].x, a.x, v0);
    v1 = fma(y[h].x, a.y, v1);
    v0 = fma(y[h].y, b.x, v0);
    v1 = fma(y[h].y, b.y, v1);
  }
  if (r < m)
    reinterpret_cast<double2 *>(X + int64_t(r) * SB_B)[c2] =
        make_double2(fma(-0.5, v0, x.x), fma(-0.5, v1, x.y));
}

// A22 -= Y W^T + W Y^T on 64 x 64 lower tiles, mirrored (A22 stays bitwise
// symmetric).  The whole K = 64 of both operands is staged at once -- A side
// [Y_rows | W_rows], B side [W_cols | Y_cols], k-major -- behind ONE barrier,
// with the tile's old values already in flight: the K = 96 kernel of the
// TSQR path (tsqr.hip syr2k_bs_kernel) waits out an L2 round trip per 16-deep
// slab.
constexpr int WT = 64, WK = 2 * SB_B, WP = 4;
static_assert(WK * (WT + WP) >= WT * (WT + 1), "mirror tile must fit");
// NP (Y, W) pairs: A22 -= sum_p Y_p W_p^T + W_p Y_p^T (NP = 2: two panels'
// updates deferred into one pass over A22, K = 128 staged 64 at a time).
struct YW2 {
  const double *Y[2], *W[2];  // m x 32 each, leading dimension SB_B
};

// Persistent: two workgroups per CU loop over the lower tiles; while a tile's
// operands are staged, multiplied and written back, the NEXT tile's old
// values are already loading (issued after this tile's operand loads, so
// waiting for those leaves them in flight).  One tile per workgroup left the
// memory pipe idle through every workgroup's MFMA, epilogue and dispatch:
// 3.7 TB/s on the HBM-resident trailing matrices of n >= 12,288.
__device__ __forceinline__ void syr2k_tile(int b, int &tm, int &tn) {
  int I = int((sqrt(8.0 * b + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= b) ++I;
  while (I * (I + 1) / 2 > b) --I;
  tm = I * WT;
  tn = (b - I * (I + 1) / 2) * WT;
}
template <int NP>
__global__ __launch_bounds__(256, 2) void syr2k_wp_kernel(double *__restrict__ A, int64_t lda,
                                                          int m, YW2 yw, int ntiles) {
  __shared__ double Aop[WK][WT + WP];
  __shared__ double Bop[WK][WT + WP];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  int b = blockIdx.x;
  if (b >= ntiles) return;
  auto load_old = [&](int tb, double (&o)[2][2][4]) __attribute__((always_inline)) {
    int tm, tn;
    syr2k_tile(tb, tm, tn);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int gi = min(tm + wm * 32 + i * 16 + (lane >> 4) + 4 * r, m - 1);
          const int gj = min(tn + wn * 32 + j * 16 + (lane & 15), m - 1);
          o[i][j][r] = A[int64_t(gi) * lda + gj];
        }
  };
  double old[2][2][4], nold[2][2][4];
  load_old(b, old);
  for (; b < ntiles; b += gridDim.x) {
    int tm, tn;
    syr2k_tile(b, tm, tn);
    const int rl = tid >> 2, k0 = (tid & 3) * 8;
    const int gr = min(tm + rl, m - 1), gc = min(tn + rl, m - 1);
    const bool okr = tm + rl < m, okc = tn + rl < m;
    doublex4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = doublex4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int pp = 0; pp < NP; ++pp) {
      // the previous tile's mirror reads / the previous pair's MFMA reads of Aop are done
      __syncthreads();
      const double *Y = yw.Y[pp], *W = yw.W[pp];
      double2 v[4][4];
      {
        const double *src[4] = {Y + int64_t(gr) * SB_B + k0, W + int64_t(gr) * SB_B + k0,
                                W + int64_t(gc) * SB_B + k0, Y + int64_t(gc) * SB_B + k0};
#pragma unroll
        for (int o = 0; o < 4; ++o)
#pragma unroll
          for (int h = 0; h < 4; ++h) v[o][h] = reinterpret_cast<const double2 *>(src[o])[h];
      }
      if (pp == 0) {
        __builtin_amdgcn_sched_barrier(0);
        const int bn = b + int(gridDim.x);
        if (bn < ntiles) load_old(bn, nold);  // in flight through this tile
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const int k = k0 + 2 * h;
        Aop[k][rl] = okr ? v[0][h].x : 0.0;
        Aop[k + 1][rl] = okr ? v[0][h].y : 0.0;
        Aop[SB_B + k][rl] = okr ? v[1][h].x : 0.0;
        Aop[SB_B + k + 1][rl] = okr ? v[1][h].y : 0.0;
        Bop[k][rl] = okc ? v[2][h].x : 0.0;
        Bop[k + 1][rl] = okc ? v[2][h].y : 0.0;
        Bop[SB_B + k][rl] = okc ? v[3][h].x : 0.0;
        Bop[SB_B + k + 1][rl] = okc ? v[3][h].y : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int kq = 0; kq < WK; kq += 4) {
        double af[2], bf[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) af[i] = Aop[kq + (lane >> 4)][wm * 32 + i * 16 + (lane & 15)];
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[j] = Bop[kq + (lane >> 4)][wn * 32 + j * 16 + (lane & 15)];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();  // operand images dead: Aop becomes the mirror tile
    double(*Tt)[WT + 1] = reinterpret_cast<double(*)[WT + 1]>(&Aop[0][0]);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int li = wm * 32 + i * 16 + (lane >> 4) + 4 * r, lj = wn * 32 + j * 16 + (lane & 15);
          const int gi = tm + li, gj = tn + lj;
          if (gi < m && gj < m && gi >= gj) {
            const double val = old[i][j][r] - acc[i][j][r];
            A[int64_t(gi) * lda + gj] = val;
            if (tm != tn) Tt[li][lj] = val;
            else if (gi != gj) A[int64_t(gj) * lda + gi] = val;
          }
        }
    if (tm != tn) {  // uniform per workgroup
      __syncthreads();
      for (int idx = tid; idx < WT * WT; idx += 256) {
        const int lc = idx >> 6, lr = idx & 63;  // row tn + lc, column tm + lr
        if (tn + lc < m && tm + lr < m) A[int64_t(tn + lc) * lda + tm + lr] = Tt[lr][lc];
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) old[i][j][r] = nold[i][j][r];
  }
}

// ---------------------------------------------------------------------------
// Panel pairs (single-level plans): the two-sided update of panel a is
// deferred and merged with panel b's (the next 32 columns) into one rank-128
// pass over the trailing matrix.
//  1. after W_a: panel b's columns (every row of A22_a, the 32 columns at its
//     left edge, lower part + mirror) get panel a's update now (they are
//     panel b's QR input and its band diagonal block);
//  2. panel b's X is formed from the NOT yet updated trailing matrix,
//     X_raw = A_cur YT_b, and corrected:  X_b = X_raw - Y_a' P - W_a' Q,
//     P = W_a'^T YT_b, Q = Y_a'^T YT_b (a' = panel a's rows below panel b's
//     columns); M_b = M_raw - T_b^T (E1 P + E2 Q), E1 = Y_b^T Y_a',
//     E2 = Y_b^T W_a' (the products ride on the X / M launch, band.hip);
//  3. one syr2k over A22_b with (Y_a', W_a') and (Y_b, W_b).
// Per pair the trailing matrix is streamed 3x (two X passes, one update of
// 1.5x the bytes) instead of 4x.
// ---------------------------------------------------------------------------
// 1: A22[i][j] -= sum_l Y[i][l] W[j][l] + W[i][l] Y[j][l] for j < 32,
// i >= j, mirrored to A22[j][i]; 32 rows x 32 columns per workgroup.
__global__ __launch_bounds__(256) void panel_upd_kernel(double *__restrict__ A, int64_t lda, int m,
                                                        const double *__restrict__ Y,
                                                        const double *__restrict__ W) {
  __shared__ double yc[SB_B][SB_B + 1], wc[SB_B][SB_B + 1];  // rows 0..31: the columns' factors
  __shared__ double yr[SB_B][SB_B + 1], wr[SB_B][SB_B + 1];  // this block's 32 rows
  const int tid = threadIdx.x, i0 = blockIdx.x * SB_B;
  for (int e = tid; e < SB_B * SB_B; e += 256) {
    const int r = e >> 5, c = e & 31;
    yc[r][c] = Y[r * SB_B + c];
    wc[r][c] = W[r * SB_B + c];
    const int gi = min(i0 + r, m - 1);
    yr[r][c] = Y[int64_t(gi) * SB_B + c];
    wr[r][c] = W[int64_t(gi) * SB_B + c];
  }
  __syncthreads();
  const int j = tid & 31;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int il = (tid >> 5) + 8 * q, i = i0 + il;
    if (i >= m || i < j) continue;
    double v = 0.0;
#pragma unroll
    for (int l = 0; l < SB_B; ++l) v = fma(yr[il][l], wc[j][l], v);
#pragma unroll
    for (int l = 0; l < SB_B; ++l) v = fma(wr[il][l], yc[j][l], v);
    const double a = A[int64_t(i) * lda + j] - v;
    A[int64_t(i) * lda + j] = a;
    if (i != j) A[int64_t(j) * lda + i] = a;
  }
}

// 2: W_b = X_raw - Ya P - Wa Q - 1/2 Yb M_b in place over X (as
// w_update_kernel, two more 32-term products); PQ = {P, Q, T^T (E1 P + E2 Q)}
// as the X / M launch leaves it.
__global__ __launch_bounds__(256) void w_update2_kernel(const double *__restrict__ Yb,
                                                        double *__restrict__ X, int m,
                                                        const double *__restrict__ M,
                                                        const double *__restrict__ Ya,
                                                        const double *__restrict__ Wa,
                                                        const double *__restrict__ PQ) {
  __shared__ double2 Ms[SB_B][SB_B / 2], Ps[SB_B][SB_B / 2], Qs[SB_B][SB_B / 2];
  const int tid = threadIdx.x;
  const int r = blockIdx.x * WU_R + (tid >> 4), c2 = tid & 15;
  const int rc = min(r, m - 1);
  for (int e = tid; e < SB_B * SB_B / 2; e += 256) {
    const double2 mr = reinterpret_cast<const double2 *>(M)[e];
    const double2 td = reinterpret_cast<const double2 *>(PQ + 2048)[e];
    Ms[e >> 4][e & 15] = make_double2(mr.x - td.x, mr.y - td.y);  // M_b = M_raw - T^T D
    Ps[e >> 4][e & 15] = reinterpret_cast<const double2 *>(PQ)[e];
    Qs[e >> 4][e & 15] = reinterpret_cast<const double2 *>(PQ + 1024)[e];
  }
  const double2 x = reinterpret_cast<const double2 *>(X + int64_t(rc) * SB_B)[c2];
  __syncthreads();
  double v0 = 0.0, v1 = 0.0, u0 = 0.0, u1 = 0.0;
  for (int h = 0; h < SB_B; ++h) {
    const double yb = Yb[int64_t(rc) * SB_B + h], ya = Ya[int64_t(rc) * SB_B + h],
                 wa = Wa[int64_t(rc) * SB_B + h];
    const double2 mm = Ms[h][c2], pp = Ps[h][c2], qq = Qs[h][c2];
    v0 = fma(yb, mm.x, v0);
    v1 = fma(yb, mm.y, v1);
    u0 = fma(ya, pp.x, u0);
    u1 = fma(ya, pp.y, u1);
    u0 = fma(wa, qq.x, u0);
    u1 = fma(wa, qq.y, u1);
  }
  if (r < m)
    reinterpret_cast<double2 *>(X + int64_t(r) * SB_B)[c2] =
        make_double2((x.x - u0) - 0.5 * v0, (x.y - u1) - 0.5 * v1);
}

}  // namespace

namespace tg {

hipError_t launch_w_update(hipStream_t st, const double *Y, double *X, int m, const double *M) {
  hipLaunchKernelGGL(w_update_kernel, dim3(cdiv(m, WU_R)), dim3(256), 0, st, Y, X, m, M);
  return hipGetLastError();
}

hipError_t launch_w_update2(hipStream_t st, const double *Yb, double *X, int m, const double *M,
                            const double *Ya, const double *Wa, const double *PQ) {
  hipLaunchKernelGGL(w_update2_kernel, dim3(cdiv(m, WU_R)), dim3(256), 0, st, Yb, X, m, M, Ya, Wa,
                     PQ);
  return hipGetLastError();
}

hipError_t launch_panel_upd(hipStream_t st, double *A22, int lda, int m, const double *Y,
                            const double *W) {
  hipLaunchKernelGGL(panel_upd_kernel, dim3(cdiv(m, SB_B)), dim3(256), 0, st, A22, int64_t(lda), m,
                     Y, W);
  return hipGetLastError();
}

hipError_t launch_syr2k(hipStream_t st, double *A22, int lda, int m, const double *Y,
                        const double *W, const double *Ya, const double *Wa) {
  const XcdInfo xi = xcd_info();
  const int ncu = std::max(1, xi.xcds * xi.cus_per_xcd);
  const int nt = cdiv(m, WT), tiles = nt * (nt + 1) / 2, np = Ya ? 2 : 1;
  auto tok = prof_begin(st, PROF_SBUPD, 12.0 * double(m) * m, 64.0 * np * double(m) * m);
  if (Ya)
    hipLaunchKernelGGL(syr2k_wp_kernel<2>, dim3(std::min(tiles, 2 * ncu)), dim3(256), 0, st, A22,
                       int64_t(lda), m, YW2{{Ya, Y}, {Wa, W}}, tiles);
  else
    hipLaunchKernelGGL(syr2k_wp_kernel<1>, dim3(std::min(tiles, 2 * ncu)), dim3(256), 0, st, A22,
                       int64_t(lda), m, YW2{{Y, nullptr}, {W, nullptr}}, tiles);
  prof_end(st, tok);
  return hipGetLastError();
}

}  // namespace tg
