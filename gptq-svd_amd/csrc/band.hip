// Stage 1 of the two-stage eigensolver: dense symmetric -> band (sy2sb).
//
// Replaces the first half of the reduction inside `torch.linalg.eigh`
// (/root/reference/src/TruncGPTQ/gptq_utils.py:92).  The one-stage dlatrd
// reduction (eigh.hip) streams the trailing matrix once per column with two
// grid-wide reductions each; here every panel of SB_B = 32 columns is
// factorised once and applied with GEMM-shaped FP64 MFMA work:
//
//   panel P = A[r0:, p:p+32]  (m = n - r0 rows)
//   Q R = P by the panel QR (pqr.hip): one compact-WY block, Y (m x 32), T
//   A22 <- Q^T A22 Q as  X = A22 Y T and M = T^T Y^T X (xm_kernel, here),
//          W = X - 1/2 Y M,  A22 -= Y W^T + W Y^T (sbupd.hip) on lower tiles,
//          mirrored, so A22 stays bitwise symmetric.
//   A[r0:, p:p+32] <- [R; 0]  (and its transpose).
//
// This file: the plan, the side stream, the X / M kernel and the production
// driver sy2sb_single.  Plans that are not `single` (panels past the panel
// QR's row limit, TG_SB_TSQR=1) take the TSQR tree of tsqr.hip.
//
// The reflectors (Y, T of every panel) stay in the workspace for the
// back-transformation Z <- Q1 Z of the eigenvectors.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "band.h"
#include "gemm64.h"
#include "reduce.h"
#include "spin.h"

namespace tg {

SbPlan::SbPlan(int n) {
  ncmax = std::max(1, n / SB_C);
  const char *e = getenv("TG_SB_TSQR");
  single = !(e && e[0] == '1') && pqr_rows_per_thread(n) > 0;
  int p = 0;
  while (p + SB_B < n - 1) {
    SbPanel P{};
    P.p = p;
    P.r0 = p + SB_B;
    P.m = n - P.r0;
    if (single) {
      P.L[0] = SbLevel{P.m, 1, ytotal, ttotal};
      ytotal += size_t(P.m) * SB_B;
      ttotal += size_t(SB_B) * SB_B;
      P.nl = 1;
      panels.push_back(P);
      p += SB_B;
      continue;
    }
    int rows = P.m, l = 0;
    while (true) {
      SbLevel &L = P.L[l];
      L.rows = rows;
      L.nc = std::max(1, rows / SB_C);
      L.yoff = ytotal;
      L.toff = ttotal;
      ytotal += size_t(rows) * SB_B;
      ttotal += size_t(L.nc) * SB_B * SB_B;
      ++l;
      if (L.nc == 1) break;
      rows = L.nc * SB_B;
    }
    P.nl = l;
    panels.push_back(P);
    p += SB_B;
  }
}

}  // namespace tg

namespace {

using tg::SB_B;

typedef double doublex4 __attribute__((ext_vector_type(4)));

// Single-level panels: X = A22 YT (m x 32, K = m) by row blocks, with the
// 32 x 32 products Y_zᵀ X_z of the blocks reduced on the way to
// M = Tᵀ (Yᵀ X) -- replaces the split-K GEMM over 256-row blocks of A22ᵀ,
// its partial sum and the separate M reduction (three launches).
// One workgroup per XR rows of X, XW waves splitting K (interleaved steps),
// each accumulating a 16 x 32 tile on FP64 MFMA with DA steps of loads in
// flight; the XW tiles are summed in wave order.  Yᵀ X partials: per
// workgroup, then per group of XG workgroups by its last arriver, then (more
// than one group) over the groups by the last group -- fixed orders, so the
// sums are bit-reproducible; the last arriver forms M.  Tickets: tick[0 ..
// groups) and tick[groups], zero before the launch, reset by their last
// arrivers.
constexpr int XR = 16, XW = 8, XG = 32;
struct XmArgs {
  const double *A;  // A22, lda
  int64_t lda;
  int m;
  const double *YT, *Y, *T;
  double *X, *part, *gpart, *M;
  unsigned *tick;
  int asm_loads;  // K loop with the hand-written loads and waits (TG_XM_ASM, default 1)
  // panel pairs (NBC = 2 only): panel a's deferred factors Ya = Y_a', Wa =
  // W_a' (rows of this panel's A22, ld 32) -> the corrections' products
  // P = Wa^T YT, Q = Ya^T YT, E1 = Y^T Ya, E2 = Y^T Wa ride on the block
  // partials and the last arriver writes PQ = {P, Q, T^T (E1 P + E2 Q)}
  // for w_update2_kernel (sbupd.hip); null: none
  const double *Ya, *Wa;
  double *PQ;
  // K split: S workgroups per column block, each over kc rows of A22 (a
  // multiple of 32); their partial X blocks meet in xpart (write-through) and
  // the last of the S (ticket cbt[cb], reset by it) sums them in split order
  // and goes on as the block's workgroup.  S = 1: no split.
  int S, kc;
  double *xpart;
  unsigned *cbt;
};
// The product is formed transposed, Xᵀ[:, j-block] = YTᵀ · A22[:, j-block]
// (A22 symmetric): the MFMA B operand is then 4 rows x 16 consecutive
// columns of A22, so lane l reads A22[k + l/16][j0 + l%16] and every load
// instruction covers four whole 128-B lines (the row-block form, A operand =
// 16 rows x 4 k, touched sixteen half-used lines per instruction and
// streamed at ~8 GB/s per CU).  The A operand is YTᵀ: lane l reads
// YT[k + l/16][16 i + l%16], 128 B of an L2-resident row.  All workgroups
// sweep K in the same order, so at any moment they read neighbouring strips
// of the same rows of A22.
// NBC 16-column blocks per workgroup (XR = 16 NBC rows of X): the YT
// fragments of a step feed all NBC blocks, so YT's L2 -> CU traffic is
// 16 m^2 / NBC bytes per panel against A22's 8 m^2.  NBC = 2 once the grid
// still covers the chip (m >= XM_WIDE).
constexpr int XM_WIDE = 6144;
// TG_XM_PACK (build-time, NBC = 2): a lane's two A22 values are adjacent
// columns (r0 + 2j, r0 + 2j + 1) and its two YT values adjacent YT columns
// (2j, 2j + 1), one 16-byte load each -- two load instructions per step
// instead of four, the same bytes.  MFMA block c then holds the columns of
// parity c and block i the YT columns of parity i; the products, their k
// order and so every X entry are unchanged, only where they land in the
// accumulators (the reduction's LDS image is written accordingly).
#ifndef TG_XM_PACK
#define TG_XM_PACK 1
#endif
#ifndef TG_XM_DA2
#define TG_XM_DA2 6
#endif
#ifndef TG_XM_MINW2
#define TG_XM_MINW2 4
#endif
// NBC = 1: TG_XM_PACK1 packs the two YT values (the single A22 value stays
// one 8-byte load), TG_XM_DA1 steps in flight
#ifndef TG_XM_PACK1
#define TG_XM_PACK1 0
#endif
#ifndef TG_XM_DA1
#define TG_XM_DA1 8
#endif
template <int NBC>
constexpr bool xm_pack() { return NBC == 2 && TG_XM_PACK; }
template <int NBC>
constexpr bool xm_pack_yt() { return NBC == 2 ? TG_XM_PACK : TG_XM_PACK1; }
typedef double xm_d2 __attribute__((ext_vector_type(2)));
template <int NBC>
struct XmStep {
  double b[NBC];
  xm_d2 ap;  // YT values (a[0], a[1])
};
template <>
struct XmStep<2> {
  xm_d2 bp, ap;  // packed: (b[0], b[1]), (a[0], a[1]) -- or unpacked, element-wise
};
template <int NBC>
__device__ __forceinline__ double xm_b(const XmStep<NBC> &f, int c) { return f.b[c]; }
template <>
__device__ __forceinline__ double xm_b<2>(const XmStep<2> &f, int c) { return f.bp[c]; }
template <int NBC>
__device__ __forceinline__ double xm_a(const XmStep<NBC> &f, int i) { return f.ap[i]; }
template <int NBC>
__device__ __forceinline__ void xm_load(const XmArgs &g, const int (&col)[NBC], int k0,
                                        XmStep<NBC> &f) {
  const int lane = threadIdx.x & 63;
  const int k = min(k0 + (lane >> 4), g.m - 1);
  if constexpr (xm_pack<NBC>()) {  // col[0] = the pair's first column
    f.bp = *reinterpret_cast<const xm_d2 *>(g.A + int64_t(k) * g.lda + col[0]);
    f.ap = *reinterpret_cast<const xm_d2 *>(g.YT + int64_t(k) * SB_B + 2 * (lane & 15));
  } else if constexpr (NBC == 2) {
    f.bp[0] = g.A[int64_t(k) * g.lda + col[0]];
    f.bp[1] = g.A[int64_t(k) * g.lda + col[1]];
    f.ap[0] = g.YT[int64_t(k) * SB_B + (lane & 15)];
    f.ap[1] = g.YT[int64_t(k) * SB_B + 16 + (lane & 15)];
  } else {
#pragma unroll
    for (int c = 0; c < NBC; ++c) f.b[c] = g.A[int64_t(k) * g.lda + col[c]];
    if constexpr (xm_pack_yt<NBC>()) {
      f.ap = *reinterpret_cast<const xm_d2 *>(g.YT + int64_t(k) * SB_B + 2 * (lane & 15));
    } else {
      f.ap[0] = g.YT[int64_t(k) * SB_B + (lane & 15)];
      f.ap[1] = g.YT[int64_t(k) * SB_B + 16 + (lane & 15)];
    }
  }
}
// The same loads as inline asm, with the waits written out (TG_XM_ASM, the
// default): with the compiler's loads the K loop's back edge carried DA
// steps of pending loads and the compiler waited for ALL of them at the loop
// header (s_waitcnt vmcnt(0) once per DA steps), so each wave had between 0
// and DA steps in flight.  Here step u's slot waits only for its own loads
// (vmcnt = the loads of the DA - 1 younger steps), so DA - 1 steps stay in
// flight across the back edge.  The waits tie the slot's registers ("+v"), so
// nothing that reads them is scheduled above the wait, and the loop exit
// drains every slot before the registers are reused.
__device__ __forceinline__ double xm_gload(const double *p) {
  double v;
  asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(v) : "v"(p));
  return v;
}
__device__ __forceinline__ xm_d2 xm_gload2(const double *p) {
  xm_d2 v;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p));
  return v;
}
template <int NBC>
__device__ __forceinline__ void xm_load_asm(const XmArgs &g, const int (&col)[NBC], int k0,
                                            XmStep<NBC> &f) {
  const int lane = threadIdx.x & 63;
  const int k = min(k0 + (lane >> 4), g.m - 1);
  if constexpr (xm_pack<NBC>()) {
    f.bp = xm_gload2(g.A + int64_t(k) * g.lda + col[0]);
    f.ap = xm_gload2(g.YT + int64_t(k) * SB_B + 2 * (lane & 15));
  } else if constexpr (NBC == 2) {
    f.bp[0] = xm_gload(g.A + int64_t(k) * g.lda + col[0]);
    f.bp[1] = xm_gload(g.A + int64_t(k) * g.lda + col[1]);
    const double *yt = g.YT + int64_t(k) * SB_B + (lane & 15);
    f.ap[0] = xm_gload(yt);
    f.ap[1] = xm_gload(yt + 16);
  } else {
#pragma unroll
    for (int c = 0; c < NBC; ++c) f.b[c] = xm_gload(g.A + int64_t(k) * g.lda + col[c]);
    if constexpr (xm_pack_yt<NBC>()) {
      f.ap = xm_gload2(g.YT + int64_t(k) * SB_B + 2 * (lane & 15));
    } else {
      const double *yt = g.YT + int64_t(k) * SB_B + (lane & 15);
      f.ap[0] = xm_gload(yt);
      f.ap[1] = xm_gload(yt + 16);
    }
  }
}
// load instructions per step slot
template <int NBC>
constexpr int xm_lps() { return xm_pack<NBC>() ? 2 : NBC + (xm_pack_yt<NBC>() ? 1 : 2); }
// wait until step slot f's loads are in: the DA - 1 younger steps' loads
// may stay outstanding
template <int NBC, int DA>
__device__ __forceinline__ void xm_wait_slot(XmStep<NBC> &f) {
  constexpr int W = (DA - 1) * xm_lps<NBC>();
  static_assert(W <= 63, "xm wait count exceeds the vmcnt field");
  if constexpr (NBC == 2) {
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(f.bp[0]), "+v"(f.bp[1]), "+v"(f.ap[0]), "+v"(f.ap[1])
                 : "n"(W));
  } else {
    asm volatile("s_waitcnt vmcnt(%3)" : "+v"(f.b[0]), "+v"(f.ap[0]), "+v"(f.ap[1]) : "n"(W));
  }
}
template <int NBC>
__device__ __forceinline__ void xm_drain_slot(XmStep<NBC> &f) {
  if constexpr (NBC == 2) {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(f.bp[0]), "+v"(f.bp[1]), "+v"(f.ap[0]), "+v"(f.ap[1]));
  } else {
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(f.b[0]), "+v"(f.ap[0]), "+v"(f.ap[1]));
  }
}
// sh (packed loads only): the lane's pair starts at column m - 1 (m odd), so
// its 16-byte load was moved one column left, (m - 2, m - 1), and column
// m - 1's value is the load's second element
template <int NBC>
__device__ __forceinline__ void xm_mma(const XmStep<NBC> &f, const bool (&cok)[NBC], bool sh,
                                       int k0, doublex4 (&acc)[NBC][2], int kend) {
  const bool kok = k0 + ((threadIdx.x & 63) >> 4) < kend;  // rows of this workgroup's K range
#pragma unroll
  for (int c = 0; c < NBC; ++c) {
    double v = xm_b<NBC>(f, c);
    if constexpr (xm_pack<NBC>())
      if (c == 0) v = sh ? xm_b<NBC>(f, 1) : v;
    const double b = (cok[c] && kok) ? v : 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
      acc[c][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(xm_a<NBC>(f, i), b, acc[c][i], 0, 0, 0);
  }
}
// sum over z in [z0, z1) of p[z * 1024 + e], in z order, with the L1-
// bypassing loads of a batch all in flight before the first add
__device__ __forceinline__ double xm_sum(const double *p, int z0, int z1, int e,
                                         int stride = 1024) {
  constexpr int NB = 8;
  double s = 0.0;
  for (int zb = z0; zb < z1; zb += NB) {
    double v[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u)
      v[u] = tg::load_partial(&p[size_t(min(zb + u, z1 - 1)) * stride + e]);
#pragma unroll
    for (int u = 0; u < NB; ++u)
      if (zb + u < z1) s += v[u];
  }
  return s;
}

// NBC = 2 (m >= XM_WIDE, the HBM-resident trailing matrices): two
// workgroups per CU -- 6 K steps in flight per wave (<= 128 registers) and
// the Y / X rows of the block staged in the reduction buffer once it is free
// (<= 80 KB of LDS), so one workgroup's reductions and ramp-up overlap the
// other's stream; at 1 per CU the stream paused through both.
template <int NBC>
constexpr int xm_depth() { return NBC == 2 ? TG_XM_DA2 : TG_XM_DA1; }
template <int NBC>
__global__ __launch_bounds__(64 * XW, NBC == 2 ? TG_XM_MINW2 : 1) void xm_kernel(XmArgs g) {
  constexpr int RB = XR * NBC;                // rows of X per workgroup
  constexpr int DA = xm_depth<NBC>();
  __shared__ double red[XW][RB][SB_B + 1];   // the last workgroup reuses it for C, T
  // the block's X and Y rows in the last two slices
  static_assert(XW >= 8, "xs and ys are red[XW - 2] and red[XW - 1]");
  double(*xs)[SB_B + 1] = red[XW - 2];
  double(*ys)[SB_B + 1] = red[XW - 1];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: uniform K loop
  // column block cb, K split ks (the S splits of a block are adjacent)
  const int cb = int(blockIdx.x) / g.S, ks = int(blockIdx.x) - cb * g.S;
  const int r0 = cb * RB;
  const int G = int(gridDim.x) / g.S, NG = (G + XG - 1) / XG;
  const int kbeg = ks * g.kc, kend = min(g.m, kbeg + g.kc);
  constexpr int YPT = RB * SB_B / (64 * XW);  // Y values per thread
  double yv[YPT];
#pragma unroll
  for (int u = 0; u < YPT; ++u) {
    const int e = tid + u * 64 * XW, rr = e >> 5, c = e & 31, row = r0 + rr;
    yv[u] = row < g.m ? g.Y[int64_t(row) * SB_B + c] : 0.0;
  }
  // wave w takes the K steps w, w + XW, ... (4 rows of A22 each) of the range
  const int KS = 4 * XW, kb = kbeg + 4 * wid;
  int colc[NBC];
  bool cok[NBC];
  // packed pair (m - 1, m) of an odd m: loaded as (m - 2, m - 1), see xm_mma
  const bool csh = xm_pack<NBC>() && r0 + 2 * (lane & 15) > g.m - 2;
#pragma unroll
  for (int c = 0; c < NBC; ++c) {
    if constexpr (xm_pack<NBC>()) {  // columns r0 + 2j + c; colc[0]: the pair, inside A22
      const int col = r0 + 2 * (lane & 15) + c;
      cok[c] = col < g.m;
      colc[c] = min(r0 + 2 * (lane & 15), g.m - 2);
    } else {
      const int col = r0 + 16 * c + (lane & 15);
      cok[c] = col < g.m;
      colc[c] = min(col, g.m - 1);
    }
  }
  doublex4 acc[NBC][2];
#pragma unroll
  for (int c = 0; c < NBC; ++c)
#pragma unroll
    for (int i = 0; i < 2; ++i) acc[c][i] = doublex4{0.0, 0.0, 0.0, 0.0};
  if (kb < kend && g.asm_loads) {
    const int nit = (kend - kb + KS - 1) / KS;
    XmStep<NBC> f[DA];
#pragma unroll
    for (int u = 0; u < DA; ++u) xm_load_asm<NBC>(g, colc, kb + KS * u, f[u]);
    for (int it = 0; it < nit; it += DA) {
#pragma unroll
      for (int u = 0; u < DA; ++u) {
        const int k0 = kb + KS * (it + u);
        xm_wait_slot<NBC, DA>(f[u]);
        xm_mma<NBC>(f[u], cok, csh, k0, acc, kend);
        xm_load_asm<NBC>(g, colc, k0 + KS * DA, f[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < DA; ++u) xm_drain_slot<NBC>(f[u]);
  } else if (kb < kend) {
    const int nit = (kend - kb + KS - 1) / KS;
    XmStep<NBC> f[DA];
#pragma unroll
    for (int u = 0; u < DA; ++u) xm_load<NBC>(g, colc, kb + KS * u, f[u]);
    // (the compiler drains vmcnt to 0 at the loop header -- the slots are
    // loop-carried -- and waits only for the slot in use inside the body;
    // unrolling 4 or 8 rounds per iteration measured no faster)
    for (int it = 0; it < nit; it += DA) {
#pragma unroll
      for (int u = 0; u < DA; ++u) {
        // scheduling barriers keep the issue order (MFMAs on step it + u,
        // then the load of step it + u + DA into the freed slot): the
        // machine scheduler otherwise sinks prefetches next to their uses
        const int k0 = kb + KS * (it + u);
        xm_mma<NBC>(f[u], cok, csh, k0, acc, kend);
        __builtin_amdgcn_sched_barrier(0);
        xm_load<NBC>(g, colc, k0 + KS * DA, f[u]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  // acc[c][i][q] = Xᵀ[16 i + lane / 16 + 4 q][r0 + 16 c + lane % 16]
#pragma unroll
  for (int c = 0; c < NBC; ++c)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if constexpr (xm_pack<NBC>())
          red[wid][2 * (lane & 15) + c][2 * ((lane >> 4) + 4 * q) + i] = acc[c][i][q];
        else if constexpr (xm_pack_yt<NBC>())
          red[wid][16 * c + (lane & 15)][2 * ((lane >> 4) + 4 * q) + i] = acc[c][i][q];
        else
          red[wid][16 * c + (lane & 15)][16 * i + (lane >> 4) + 4 * q] = acc[c][i][q];
  __syncthreads();
  double xv[YPT];
#pragma unroll
  for (int u = 0; u < YPT; ++u) {
    const int e = tid + u * 64 * XW, rr = e >> 5, c = e & 31;
    double x = 0.0;
#pragma unroll
    for (int w = 0; w < XW; ++w) x += red[w][rr][c];
    xv[u] = x;
  }
  if (g.S > 1) {
    // this split's partial X block, write-through; the last of the block's
    // S splits sums them in split order and goes on
    double *mine = g.xpart + (size_t(cb) * g.S + ks) * (RB * SB_B);
#pragma unroll
    for (int u = 0; u < YPT; ++u)
      __hip_atomic_store(&mine[tid + u * 64 * XW], xv[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0)
      s_last = __hip_atomic_fetch_add(&g.cbt[cb], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
               unsigned(g.S - 1);
    __syncthreads();
    if (!s_last) return;
    if (tid == 0) tg::ctl_reset(&g.cbt[cb]);
    const double *blk = g.xpart + size_t(cb) * g.S * (RB * SB_B);
#pragma unroll
    for (int u = 0; u < YPT; ++u) {
      const int e = tid + u * 64 * XW;
      double x = 0.0;
      for (int z = 0; z < g.S; ++z)
        x += __hip_atomic_load(&blk[size_t(z) * (RB * SB_B) + e], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
      xv[u] = x;
    }
  }
#pragma unroll
  for (int u = 0; u < YPT; ++u) {
    const int e = tid + u * 64 * XW, rr = e >> 5, c = e & 31;
    if (r0 + rr < g.m) g.X[int64_t(r0 + rr) * SB_B + c] = xv[u];
    xv[u] = r0 + rr < g.m ? xv[u] : 0.0;
  }
  __syncthreads();  // red is free: its first two slices take the block's X and Y rows
#pragma unroll
  for (int u = 0; u < YPT; ++u) {
    const int e = tid + u * 64 * XW, rr = e >> 5, c = e & 31;
    xs[rr][c] = xv[u];
    ys[rr][c] = yv[u];
  }
  // panel pairs: the block's rows of Ya, Wa and YT in the next three slices
  const bool pp = NBC == 2 && g.Ya != nullptr;  // uniform
  const int NP = pp ? 5 : 1;
  if constexpr (NBC == 2) {
    if (pp) {
#pragma unroll
      for (int u = 0; u < YPT; ++u) {
        const int e = tid + u * 64 * XW, rr = e >> 5, c = e & 31, row = r0 + rr;
        const bool ok = row < g.m;
        const int64_t o = int64_t(ok ? row : 0) * SB_B + c;
        red[2][rr][c] = ok ? g.Ya[o] : 0.0;
        red[3][rr][c] = ok ? g.Wa[o] : 0.0;
        red[4][rr][c] = ok ? g.YT[o] : 0.0;
      }
    }
  }
  __syncthreads();
  // this block's Y_zᵀ X_z (and the pair products), write-through, then the group ticket
  double *mypart = g.part + size_t(cb) * NP * 1024;
  for (int e = tid; e < SB_B * SB_B; e += 64 * XW) {
    const int a = e >> 5, c = e & 31;
    double p = 0.0;
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) p = fma(ys[rr][a], xs[rr][c], p);
    __hip_atomic_store(&mypart[e], p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if constexpr (NBC == 2) {
    if (pp) {
      // k = 0: P = Wa^T YT, 1: Q = Ya^T YT, 2: E1 = Y^T Ya, 3: E2 = Y^T Wa
      for (int e = tid; e < 4 * SB_B * SB_B; e += 64 * XW) {
        const int k = e >> 10, a = (e >> 5) & 31, c = e & 31;
        const double(*L)[SB_B + 1] = k == 0 ? red[3] : k == 1 ? red[2] : ys;
        const double(*R)[SB_B + 1] = k <= 1 ? red[4] : k == 2 ? red[2] : red[3];
        double p = 0.0;
#pragma unroll
        for (int rr = 0; rr < RB; ++rr) p = fma(L[rr][a], R[rr][c], p);
        __hip_atomic_store(&mypart[1024 + e], p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const int grp = cb / XG, z0 = grp * XG, z1 = min(G, z0 + XG);
  if (tid == 0)
    s_last = __hip_atomic_fetch_add(&g.tick[grp], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
             unsigned(z1 - z0 - 1);
  __syncthreads();
  if (!s_last) return;
  // Cs = C (Y^T X), then the pair sums P, Q, E1, E2 (pp); Ts = T
  double *Cs = &red[0][0][0], *Ts = Cs + 5 * SB_B * SB_B;
  static_assert(XW * XR * (SB_B + 1) >= 2 * SB_B * SB_B, "C and T fit in red");
  static_assert(NBC == 1 || XW * XR * NBC * (SB_B + 1) >= 6 * SB_B * SB_B,
                "C, the pair sums and T fit in red");
  if (!pp) Ts = Cs + SB_B * SB_B;
  const int ne = NP * SB_B * SB_B;
  for (int e = tid; e < ne; e += 64 * XW) {
    const double s = xm_sum(g.part, z0, z1, e, NP * 1024);
    if (NG == 1)
      Cs[e] = s;  // one group: its last arriver forms M (no second hand-off)
    else
      __hip_atomic_store(&g.gpart[size_t(grp) * NP * 1024 + e], s, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  }
  for (int e = tid; e < SB_B * SB_B; e += 64 * XW) Ts[e] = g.T[e];
  if (NG > 1) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      tg::ctl_reset(&g.tick[grp]);
      s_last = __hip_atomic_fetch_add(&g.tick[NG], 1u, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT) == unsigned(NG - 1);
    }
    __syncthreads();
    if (!s_last) return;
    for (int e = tid; e < ne; e += 64 * XW) Cs[e] = xm_sum(g.gpart, 0, NG, e, NP * 1024);
  }
  __syncthreads();
  for (int e = tid; e < SB_B * SB_B; e += 64 * XW) {
    const int a = e >> 5, c = e & 31;
    double v = 0.0;
    for (int k = 0; k <= a; ++k) v = fma(Ts[k * SB_B + a], Cs[k * SB_B + c], v);
    g.M[e] = v;
  }
  if (pp) {
    // PQ[0 .. 2047] = {P, Q}; D = E1 P + E2 Q into C's slot (M is out);
    // PQ[2048 ..] = T^T D
    const double *Ps = Cs + 1024, *Qs = Cs + 2048, *E1 = Cs + 3072, *E2 = Cs + 4096;
    for (int e = tid; e < 2048; e += 64 * XW) g.PQ[e] = Cs[1024 + e];
    __syncthreads();
    for (int e = tid; e < SB_B * SB_B; e += 64 * XW) {
      const int a = e >> 5, c = e & 31;
      double v = 0.0;
#pragma unroll 8
      for (int k = 0; k < SB_B; ++k) v = fma(E1[a * SB_B + k], Ps[k * SB_B + c], v);
#pragma unroll 8
      for (int k = 0; k < SB_B; ++k) v = fma(E2[a * SB_B + k], Qs[k * SB_B + c], v);
      Cs[e] = v;
    }
    __syncthreads();
    for (int e = tid; e < SB_B * SB_B; e += 64 * XW) {
      const int a = e >> 5, c = e & 31;
      double v = 0.0;
      for (int k = 0; k <= a; ++k) v = fma(Ts[k * SB_B + a], Cs[k * SB_B + c], v);
      g.PQ[2048 + e] = v;
    }
  }
  if (tid == 0) {
    tg::ctl_reset(&g.tick[grp]);
    if (NG > 1) tg::ctl_reset(&g.tick[NG]);
  }
}

}  // namespace

namespace tg {

constexpr int NPQ_STAT = 8;

hipError_t side_stream(SideStream *&out) {
  static SideStream ss[64];
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  SideStream &x = ss[dev & 63];
  if (!x.s) {
    if ((e = hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking)) != hipSuccess) return e;
    for (int i = 0; i < 2; ++i) {
      if ((e = hipEventCreateWithFlags(&x.ev0[i], hipEventDisableTiming)) != hipSuccess) return e;
      if ((e = hipEventCreateWithFlags(&x.ev1[i], hipEventDisableTiming)) != hipSuccess) return e;
    }
    if ((e = hipEventCreateWithFlags(&x.evj, hipEventDisableTiming)) != hipSuccess) return e;
  }
  out = &x;
  return hipSuccess;
}

// Fork work onto the side stream after everything queued on st so far, and
// join it back (tg_eigh_vectors_range: the Q2 T factors beside inverse
// iteration)
hipError_t side_fork(hipStream_t st, hipStream_t *side) {
  SideStream *ss = nullptr;
  TG_CHK(side_stream(ss));
  TG_CHK(hipEventRecord(ss->evj, st));
  TG_CHK(hipStreamWaitEvent(ss->s, ss->evj, 0));
  *side = ss->s;
  return hipSuccess;
}
hipError_t side_join(hipStream_t st) {
  SideStream *ss = nullptr;
  TG_CHK(side_stream(ss));
  TG_CHK(hipEventRecord(ss->evj, ss->s));
  TG_CHK(hipStreamWaitEvent(st, ss->evj, 0));
  return hipSuccess;
}

// X = A22 YT and M = T^T Y^T X in one launch (row blocks of A22)
static int xm_nbc(int m) {
  const char *fx = getenv("TG_XM_NBC");  // development switch (1 | 2), read per call
  return fx ? (atoi(fx) == 2 ? 2 : 1) : (m >= XM_WIDE ? 2 : 1);
}
// K splits per column block (TG_XM_KSPLIT=s forces s, 1 = none, 0 = the
// default; read per call): the column-block grid alone leaves CUs idle once m / (16 NBC) is
// below the device's workgroup slots, and at m / 32 = 192 .. 384 blocks of
// the HBM-resident NBC = 2 launches it puts two blocks on some CUs and one on
// others.  Splitting K brings the grid to about three rounds of 512
// workgroups (two per CU on 256 CUs) -- a function of m only, so the
// results do not depend on the device.
// Measured (profiles/r06/env_ab_*_ksplit.log): n = 12,288 392.8 -> 389.7 ms
// (the NBC = 2 launches 244 -> 226 us), but n = 4096 56.96 -> 58.30 ms (the
// 16-column launches are MALL-resident and their extra partial hand-off
// costs more than the balance gains), so only the 32-column form splits.
static int xm_ksplit(int m, int G, int nbc) {
  const char *e = getenv("TG_XM_KSPLIT");  // 0 / unset: the default below
  int S = (e && atoi(e) > 0) ? atoi(e) : (nbc == 1 || G >= 1536 ? 1 : cdiv(1536, G));
  S = std::max(1, std::min(8, S));
  while (S > 1 && cdiv(m, S) < 4 * 32) --S;  // at least 128 rows per split
  return S;
}
// Ya / Wa (a pair's partner): the 32-column form (only it carries the pair
// products), which also writes the products into PQ.
static hipError_t launch_xm(hipStream_t st, double *A22, int lda, int m, const double *YT,
                            const double *Yp, const double *Tp, double *X, const SbBufs &b,
                            int n, const double *Ya = nullptr, const double *Wa = nullptr,
                            double *PQ = nullptr) {
  const int nbc = Ya ? 2 : xm_nbc(m);
  const int G = cdiv(m, XR * nbc), np = Ya ? 5 : 1;
  const int S = xm_ksplit(m, G, nbc), kc = cdiv(cdiv(m, S), 32) * 32;
  const char *xs = getenv("TG_XM_ASM");  // development switch: 0 = compiler-scheduled loads
  const int asm_loads = !(xs && xs[0] == '0');
  XmArgs xa{A22, int64_t(lda), m, YT, Yp, Tp, X, b.U, b.U + size_t(G) * np * 1024, b.M,
            b.xm_tick, asm_loads, Ya, Wa, PQ, S, kc, b.xm_xpart, b.xm_tick + xm_cbt_off(n)};
  if (nbc == 2) hipLaunchKernelGGL(xm_kernel<2>, dim3(G * S), dim3(64 * XW), 0, st, xa);
  else hipLaunchKernelGGL(xm_kernel<1>, dim3(G * S), dim3(64 * XW), 0, st, xa);
  return hipGetLastError();
}

// Panel pairs (see panel_upd_kernel) for panels whose partner has at least
// PAIR_MIN trailing rows (TG_SB_PAIR=1: every panel with a partner of >= 256
// rows, 0: none; read per call); the workspace's X holds n x ncmax*32
// doubles, so two m x 32 slabs fit once n >= 2 SB_C.  The merged rank-128
// update streams the HBM-resident trailing matrix once per two panels; the
// pair's correction products ride on the partner's X / M launch.  Measured
// (tools/solve_time.py): n = 12,288 509.5 vs 521.8 ms, n = 28,672 3.18 vs
// 3.47 s, but n = 4096 64.6 vs 61.4 ms (MALL-resident trailing matrices: the
// corrections' reductions cost more than the pass they save), hence the
// 6144-row default.
constexpr int PAIR_MIN_ALL = 256, PAIR_MIN = 6144;
// a default pair's partner is at the width where xm_kernel<2> is the default
// form anyway: forming the products there changes no production launch
static_assert(PAIR_MIN >= XM_WIDE, "default pairs take xm_kernel<2> by their width");

// One compact-WY block per panel (pqr.hip): panel QR, X = A22 YT, M, update.
// (Measured and removed in round 3's clean-up, DESIGN.md §5: a look-ahead
// with the next panel's QR on a side stream, +5 ms -- the QR's workgroups need
// a whole CU's LDS and wait for the trailing update to drain; the same on
// CU-masked streams, update kernels 1.3-2x slower; A22 kept as its lower
// triangle, X 27 -> 35 us for syr2k 38 -> 35 us.  Round 5: the look-ahead
// with the update's workgroups kept off the QR's XCD (b % 8 != 0, dense
// tile index) does overlap the two, but the next panel's column update and
// the cross-stream waits cost what the overlap saves: 59.11 vs 59.11 ms at
// n = 4096, +2 ms at 12,288.)
static hipError_t sy2sb_single(hipStream_t st, double *A, int lda, int n, const SbPlan &pl,
                               const SbBufs &b) {
  TG_CHK(hipMemsetAsync(b.pq_ctl, 0, sizeof(unsigned) * pq_ctl_words(n), st));
  TG_CHK(hipMemsetAsync(b.xm_tick, 0, sizeof(unsigned) * xm_tick_words(n), st));
  const int np = int(pl.panels.size());
  const char *pe = getenv("TG_SB_PAIR");
  const bool pairs = !(pe && pe[0] == '0') && pl.ncmax >= 2;
  const int pair_min = (pe && pe[0] == '1') ? PAIR_MIN_ALL : PAIR_MIN;
  double *Xa = b.X, *Xb = b.X + size_t(n) * SB_B;
  for (int pi = 0; pi < np; ++pi) {
    const SbPanel &P = pl.panels[pi];
    const int m = P.m;
    double *A22 = A + int64_t(P.r0) * lda + P.r0;
    double *Yp = b.Y + P.L[0].yoff, *Tp = b.T + P.L[0].toff;
    TG_CHK(panel_qr(st, A, lda, P.p, P.r0, P.m, Yp, b.YT, Tp, b.pq_part, b.pq_bc,
                    b.pq_ctl + 4 + 4 * pi, b.pq_ctl));
    TG_CHK(launch_xm(st, A22, lda, m, b.YT, Yp, Tp, Xa, b, n));
    TG_CHK(launch_w_update(st, Yp, Xa, m, b.M));  // W = X - Y M / 2 in place
    if (!(pairs && pi + 1 < np && pl.panels[pi + 1].m >= pair_min)) {
      TG_CHK(launch_syr2k(st, A22, lda, m, Yp, Xa));  // A22 -= Y W^T + W Y^T
      continue;
    }
    // panel b = pi + 1: its columns get panel a's update now
    TG_CHK(launch_panel_upd(st, A22, lda, m, Yp, Xa));
    ++pi;
    const SbPanel &Q = pl.panels[pi];
    const int mb = Q.m;
    double *A22b = A + int64_t(Q.r0) * lda + Q.r0;
    double *Yb = b.Y + Q.L[0].yoff, *Tb = b.T + Q.L[0].toff;
    const double *Ya = Yp + SB_B * SB_B, *Wa = Xa + SB_B * SB_B;  // panel a's rows >= Q.r0
    TG_CHK(panel_qr(st, A, lda, Q.p, Q.r0, Q.m, Yb, b.YT, Tb, b.pq_part, b.pq_bc,
                    b.pq_ctl + 4 + 4 * pi, b.pq_ctl));
    // X_raw, M_raw and the corrections' products (into G) in one launch
    TG_CHK(launch_xm(st, A22b, lda, mb, b.YT, Yb, Tb, Xb, b, n, Ya, Wa, b.G));
    TG_CHK(launch_w_update2(st, Yb, Xb, mb, b.M, Ya, Wa, b.G));
    TG_CHK(launch_syr2k(st, A22b, lda, mb, Yb, Xb, Ya, Wa));  // both panels, rank 128
  }
  return hipSuccess;
}

hipError_t sy2sb_timed_out(hipStream_t st, const SbPlan &pl, const SbBufs &b, bool *tmo) {
  *tmo = false;
  if (!pl.single || pl.panels.empty()) return hipSuccess;
  unsigned h = 0;
  hipError_t e = hipMemcpyAsync(&h, b.pq_ctl, sizeof(unsigned), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  *tmo = h != 0u;
  if (getenv("TG_PQR_STATS")) {
    std::vector<unsigned> c(4 + 4 * pl.panels.size());
    (void)hipMemcpy(c.data(), b.pq_ctl, sizeof(unsigned) * c.size(), hipMemcpyDeviceToHost);
    int hist[4][NPQ_STAT] = {};
    for (size_t i = 0; i < pl.panels.size(); ++i) {
      const unsigned v = c[4 + 4 * i + 1];
      hist[std::min(3u, v / 16)][std::min(unsigned(NPQ_STAT - 1), v % 16)]++;
    }
    fprintf(stderr, "pqr: %zu panels; accept after 2/3/4 passes: %d/%d/%d; fallback: %d\n",
            pl.panels.size(), hist[2][2], hist[2][3], hist[2][4],
            hist[3][0] + hist[3][1] + hist[3][2] + hist[3][3] + hist[3][4]);
  }
  return e;
}

hipError_t sy2sb(hipStream_t st, double *A, int lda, int n, const SbPlan &pl, const SbBufs &b) {
  return pl.single ? sy2sb_single(st, A, lda, n, pl, b) : sy2sb_tsqr(st, A, lda, pl, b);
}

hipError_t sb_apply_q1(hipStream_t st, int n, double *Z, int k, const SbPlan &pl,
                       const SbBufs &b) {
  (void)n;
  if (!pl.single) return sb_apply_q1_tsqr(st, Z, k, pl, b);
  // Z[r0:, :] -= Y (T (Y^T Z[r0:, :])) per panel, last panel first
  for (auto it = pl.panels.rbegin(); it != pl.panels.rend(); ++it) {
    const SbPanel &P = *it;
    double *Zs = Z + int64_t(P.r0) * k;
    const double *Yp = b.Y + P.L[0].yoff, *Tp = b.T + P.L[0].toff;
    auto tok = prof_begin(st, PROF_Q1, 24.0 * double(P.m) * k, 4.0 * double(P.m) * SB_B * k);
    const int splits = std::max(1, std::min(pl.ncmax, P.m / SB_C));
    TG_CHK(dgemm_splitk(st, true, false, SB_B, k, P.m, 1.0, Yp, SB_B, Zs, k, 0.0, b.P, k, splits,
                        b.Zg));
    TG_CHK(dgemm(st, false, false, SB_B, k, SB_B, 1.0, Tp, SB_B, b.P, k, 0.0, b.Mz, k));
    TG_CHK(dgemm(st, false, false, P.m, k, SB_B, -1.0, Yp, SB_B, b.Mz, k, 1.0, Zs, k));
    prof_end(st, tok);
  }
  return hipSuccess;
}

}  // namespace tg
