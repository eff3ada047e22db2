// Pivot order and R_x of the truncated spectral factorisation (A4):
// tg_pivoted_factor, tg_pivoted_factor_complement.  The U factors (A5) are in
// ufactor.hip.
//
// Replaces, in the reference's gptq_utils.py:
//   H_sqrt = S[:, None] * Vh; jax.scipy.linalg.qr(H_sqrt, pivoting=True)  :112-117
//       (XLA -> MAGMA dgeqp3)                      -> tg_pivoted_factor
//
// Pivot order.  dgeqp3 picks, at step i, the remaining column of largest
// residual norm (first index on ties) and swaps it into position i.  The
// residual column norms of S_k after i Householder steps equal the diagonal
// of the Schur complement of H_k = S_k^T S_k after i pivoted Cholesky steps,
// and the R factor equals the pivoted Cholesky factor (both with positive
// diagonal).  So the pivot sequence (identical swap bookkeeping) and R_x come
// from a greedy diagonal-pivoted Cholesky of H_k (SYRK on FP64 MFMA) in panels
// of up to PB = 32 steps.
//
// n <= 32768: the candidate-set path.  One workgroup picks a whole panel's
// pivots among the rows of largest Schur diagonal (piv_sel_kernel: 256, 512
// or 1024 candidates, the level chosen panel by panel), the panel's L columns
// and diagonals of every row are computed by fill workers in the same launch
// as the steps go (piv_stream_worker; piv_fill_kernel fills what they left,
// or everything with TG_PIV_STREAM=0), and a rank-32
// update on FP64 MFMA writes the next Schur complement, compacted to the
// unpivoted rows and stored as its lower triangle only, into the other of two
// n x n buffers (syrk_compact_p_kernel).
// n > 32768 (or TG_PIVOT_OLD=1): the old path on one n x n buffer in original
// row order.  One launch per pivot (piv_step_kernel) above 32768; below, a
// panel's steps run in one cross-workgroup launch (piv_panel_kernel) unless
// TG_PIVOT_STEPWISE=1.  A full dsyrk_tn Schur update follows each panel.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "../../include/truncgptq.h"
#include "common.h"
#include "spin.h"
#include "gemm64.h"
#include "reduce.h"

namespace {

constexpr int PB = 32;    // pivoted-Cholesky panel (steps between Schur updates)
constexpr int PGMAX = 64; // max workgroups of the per-pivot kernel

struct PivWs {
  double *B;     // k x n  S_k-scaled eigenvectors (H_sqrt)
  double *Hk;    // n x n  H_k, then its Schur complements
  double *dsc;   // n      Schur diagonal (by original index)
  double *L;     // n x k  L[r][i] (original row index r, pivot step i)
  double *LT;    // PB x n current panel of L, column-major (coalesced per step)
  double *part;  // 2 x PGMAX
  int32_t *perm; // n      position -> original index
  int32_t *pos;  // n      original index -> position
  unsigned *cnt;
  double *pp;    // PGMAX x PPS  per-workgroup step partials (value, position, row, L row)
  double *bc;    // PPS          last arriver's broadcast (pivot, its L row, swap)
  unsigned *flag;
  // candidate-set pivoting (piv_sel_kernel / piv_fill_kernel)
  int32_t *sstate;  // [0] steps done, [1] steps of the last panel, [2..] level words (SS_*)
  int32_t *prow;    // PB  pivot rows of the panel
  double *pinv;     // PB  1 / L[piv][step]
  double *Lpp;      // PB x PB  L rows of the panel's pivots (panel columns)
  double *Hk2;      // n x n  second buffer: the compacted Schur complements alternate
  int32_t *oidx;    // n  new position ps + x -> its compact index in the panel's H_k
  // streamed fill (piv_stream_worker): with prow / pinv / Lpp the ring of step records
  unsigned long long *strm;  // [0] progress word of the panel in flight (SW_*)
  int32_t *ppoi;             // PB  compact index of each pivot in the panel's H_k
  int32_t *pq;               // PB  position each pivot was swapped in from
  int32_t *fdone;            // ceil(n / 64)  launch number of the panel whose worker filled the chunk
};
constexpr int PPS = PB + 8;  // partial / broadcast record (doubles)
static_assert(PGMAX * PPS % 256 == 0, "slot copy assumes whole rounds of 256 threads");

// The candidate-set pivot order with compacted Schur complements (two n x n
// buffers) for n <= 32768; above (or TG_PIVOT_OLD=1, read per call) the
// cross-workgroup per-pivot path, which needs only one.
inline bool compact_pivot(int n) { return n <= 32768 && getenv("TG_PIVOT_OLD") == nullptr; }

template <class A>
void piv_layout(A &ar, int n, int k, PivWs *p) {
  PivWs d{};
  PivWs &q = p ? *p : d;
  auto take = [&](auto *&dst, size_t cnt) {
    using T = std::remove_reference_t<decltype(*dst)>;
    dst = ar.template take<T>(cnt);
  };
  // the two compacted H_k buffers on 2 MB boundaries (their rows are
  // gathered by the candidate steps and the fill kernel)
  auto take2m = [&](double *&dst, size_t cnt) {
    constexpr size_t AL = size_t(2) << 20;
    dst = ar.template take_aligned<double>(cnt, AL);
  };
  take(q.B, size_t(k) * n);
  take(q.pp, size_t(2) * PGMAX * PPS);
  take(q.bc, PPS);
  take(q.flag, 16);
  take2m(q.Hk, size_t(n) * n);
  take(q.dsc, n);
  take(q.L, size_t(n) * k);
  take(q.LT, size_t(PB) * n);
  take(q.part, PGMAX * 2);
  take(q.perm, n);
  take(q.pos, n);
  take(q.cnt, 16);
  take(q.sstate, 16);
  take(q.prow, PB);
  take(q.pinv, PB);
  take(q.Lpp, PB * PB);
  take2m(q.Hk2, compact_pivot(n) ? size_t(n) * n : size_t(1));
  take(q.oidx, n);
  take(q.strm, 2);
  take(q.ppoi, PB);
  take(q.pq, PB);
  take(q.fdone, size_t(tg::cdiv(n, 64)));
}

// B[t][c] = S[t] * Vh[t][c]    (gptq_utils.py:112)
__global__ void scale_rows_kernel(const double *__restrict__ Vh, int ldv, const double *__restrict__ S,
                                  int n, int k, double *__restrict__ B) {
  const int t = blockIdx.y;
  const double s = S[t];
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x)
    B[size_t(t) * n + c] = s * Vh[size_t(t) * ldv + c];
}

// (value, position) argmax with first-position tie break, published for the
// last workgroup, which then swaps perm[i] <-> perm[q].
__device__ inline void argmax_publish(double bv, int bp, int i, int n, PivWs w) {
  __shared__ double sv[256];
  __shared__ int sp[256];
  __shared__ double vals[2];
  const int tid = threadIdx.x;
  sv[tid] = bv;
  sp[tid] = bp;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
      const double ov = sv[tid + off];
      const int op = sp[tid + off];
      if (ov > sv[tid] || (ov == sv[tid] && op < sp[tid])) {
        sv[tid] = ov;
        sp[tid] = op;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    vals[0] = sv[0];
    vals[1] = double(sp[0]);
  }
  __syncthreads();
  if (tg::publish_partials(vals, 2, w.part, w.cnt)) {
    if (tid < 64) {  // one wave: lanes cover the partials, fixed butterfly argmax
      const int G = int(gridDim.x);
      double best = -INFINITY;
      int q = n;
      for (int g = tid; g < G; g += 64) {
        const double v = tg::load_partial(&w.part[g]);
        const int p = int(tg::load_partial(&w.part[G + g]));
        if (v > best || (v == best && p < q)) {
          best = v;
          q = p;
        }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best, off);
        const int op = __shfl_xor(q, off);
        if (ov > best || (ov == best && op < q)) {
          best = ov;
          q = op;
        }
      }
      if (tid == 0) {
        if (q < n && q != i) {
          const int a = w.perm[i], b = w.perm[q];
          w.perm[i] = b;
          w.perm[q] = a;
          w.pos[b] = i;
          w.pos[a] = q;
        }
        *w.cnt = 0u;
      }
    }
  }
}

// dsc = diag(Hk), perm = identity, first pivot swapped into position 0.
__global__ __launch_bounds__(256) void piv_init_kernel(int n, PivWs w) {
  double bv = -INFINITY;
  int bp = n;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    const double v = w.Hk[size_t(j) * n + j];
    w.dsc[j] = v;
    w.perm[j] = j;
    w.pos[j] = j;
    if (v > bv || (v == bv && j < bp)) {
      bv = v;
      bp = j;
    }
  }
  argmax_publish(bv, bp, 0, n, w);
}

// One pivot step i (pivot already swapped into position i).  Threads walk the
// rows in ORIGINAL order (coalesced row of H_k, panel of L^T, Schur diagonal);
// rows already pivoted (pos <= i) are skipped; the argmax breaks ties on the
// dgeqp3 position.
__global__ __launch_bounds__(256) void piv_step_kernel(int n, int k, int i, int ps, PivWs w) {
  __shared__ double lp[PB];
  const int t = i - ps;
  const int piv = w.perm[i];
  const double dpiv = w.dsc[piv];
  const double ljj = sqrt(fmax(dpiv, 0.0));
  if (threadIdx.x < t) lp[threadIdx.x] = w.LT[size_t(threadIdx.x) * n + piv];
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    w.L[size_t(piv) * k + i] = ljj;
    w.LT[size_t(t) * n + piv] = ljj;
  }
  const double inv = ljj > 0.0 ? 1.0 / ljj : 0.0;
  double bv = -INFINITY;
  int bp = n;
  const double *hrow = w.Hk + size_t(piv) * n;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
    const int pr = w.pos[r];
    double v = hrow[r];
    double lr[PB];
#pragma unroll
    for (int l = 0; l < PB; ++l) lr[l] = l < t ? w.LT[size_t(l) * n + r] : 0.0;
#pragma unroll
    for (int l = 0; l < PB; ++l) v -= l < t ? lr[l] * lp[l] : 0.0;
    if (pr <= i) continue;
    const double lv = v * inv;
    w.L[size_t(r) * k + i] = lv;
    w.LT[size_t(t) * n + r] = lv;
    const double dn = w.dsc[r] - lv * lv;
    w.dsc[r] = dn;
    if (dn > bv || (dn == bv && pr < bp)) {
      bv = dn;
      bp = pr;
    }
  }
  // dgeqp3 stops after min(k, n) steps: no swap into position k.
  if (i + 1 < k) argmax_publish(bv, bp, i + 1, n, w);
}

// Persistent form of the pivot steps of one panel (steps ps .. pe-1): one
// launch instead of one per pivot.  Thread (block b, lane x) owns rows
// r = (b * 256 + x) + u * G * 256 (u < RPT) and keeps their panel of L in
// registers.  Per step every workgroup publishes its best candidate (Schur
// diagonal, dgeqp3 position, row, and that row's panel of L) with sc1 stores
// and takes an arrival ticket; the last arriver does dgeqp3's swap
// bookkeeping and broadcasts the next pivot (its diagonal, row and L panel)
// plus the swapped pair; the others poll the broadcast flag.  All
// cross-workgroup data moves by sc1 stores + vmcnt(0) + flag/ticket and sc1
// loads (MI355X_MICROARCH.md "Valid forms"), so placement does not matter.
__device__ inline double ld1(const double *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void st1(double *p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline int ld1i(const int32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void st1i(int32_t *p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}


// Wave argmax without the LDS crossbar: partner values through
// v_permlane{32,16}_swap (lane ^ 32, ^ 16) and DPP row mirrors / quad perms
// (lane ^ 15, ^ 7, ^ 3, ^ 1); each pairing flips a new lane bit, so after the
// six stages every lane holds the maximum of the strict total order used.
__device__ inline int part32(int x) {
  const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return (threadIdx.x & 32) ? r[0] : r[1];
}
__device__ inline int part16(int x) {
  const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
  return (threadIdx.x & 16) ? r[0] : r[1];
}
template <int CTRL>
__device__ inline int partdpp(int x) {
  return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, false);
}
template <int S>
__device__ inline int partner(int x) {
  if constexpr (S == 0) return part32(x);
  else if constexpr (S == 1) return part16(x);
  else if constexpr (S == 2) return partdpp<0x140>(x);  // row_mirror: lane ^ 15
  else if constexpr (S == 3) return partdpp<0x141>(x);  // row_half_mirror: lane ^ 7
  else if constexpr (S == 4) return partdpp<0x1B>(x);   // quad_perm [3,2,1,0]: lane ^ 3
  else return partdpp<0xB1>(x);                         // quad_perm [1,0,3,2]: lane ^ 1
}
// (value desc, then p asc, then g asc): the dgeqp3 pivot rule with a
// deterministic workgroup tie-break
template <int S>
__device__ inline void argmax_stage(double &v, int &p, int &g) {
  const double ov = __hiloint2double(partner<S>(__double2hiint(v)), partner<S>(__double2loint(v)));
  const int op = partner<S>(p), og = partner<S>(g);
  if (ov > v || (ov == v && (op < p || (op == p && og < g)))) {
    v = ov;
    p = op;
    g = og;
  }
}
__device__ inline void wave_argmax(double &v, int &p, int &g) {
  argmax_stage<0>(v, p, g);
  argmax_stage<1>(v, p, g);
  argmax_stage<2>(v, p, g);
  argmax_stage<3>(v, p, g);
  argmax_stage<4>(v, p, g);
  argmax_stage<5>(v, p, g);
}

// Worker selection: the launch has at least 8 (G - 1) + 1 workgroups; each
// takes a ticket on its XCD (HW_REG_XCC_ID) and the first XCD to hand out G
// tickets becomes the worker set (pigeonhole: one always does); the others
// exit.  Workers then hand data over through that XCD's L2: plain stores +
// vmcnt(0) + agent atomic ticket, sc1 (L1-bypassing) loads.
template <int RPT>
__global__ __launch_bounds__(256) void piv_panel_kernel(int n, int k, int ps, int pe, int G,
                                                        unsigned base, PivWs w) {
  extern __shared__ int permL[];  // n: position -> row (every workgroup keeps a copy)
  __shared__ double sv[4], lrow[PB + 1];
  __shared__ int spos[4], swin[4], s_g, s_me;
  __shared__ double s_best;
  __shared__ double slotc[PGMAX * PPS];
  __shared__ double wrow[4][PB + 1];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid == 0) {
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x));
    unsigned *xc = w.flag + 4;  // [0..7] tickets per XCD, [8] chosen XCD + 1
    const unsigned tk = __hip_atomic_fetch_add(xc + (x & 7), 1u, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
    int me = -1;
    if (tk < unsigned(G)) {
      if (tk == unsigned(G) - 1) {
        unsigned expect = 0;
        __hip_atomic_compare_exchange_strong(xc + 8, &expect, x + 1, __ATOMIC_RELAXED,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      unsigned ch;
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      while ((ch = __hip_atomic_load(xc + 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u) {
        __builtin_amdgcn_s_sleep(1);
        if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ull) break;
      }
      if (ch == x + 1) me = int(tk);
    }
    s_me = me;
  }
  __syncthreads();
  const int me = s_me;
  if (me < 0) return;
  for (int x = tid; x < n; x += 256) permL[x] = w.perm[x];
  // base = arrivals of earlier panel launches (G per step before ps), from the host
  int rows[RPT], posr[RPT];
  double dsr[RPT], lr[RPT][PB];
#pragma unroll
  for (int u = 0; u < RPT; ++u) {
    rows[u] = me * 256 + tid + u * G * 256;
    const bool ok = rows[u] < n;
    posr[u] = ok ? w.pos[rows[u]] : n;
    dsr[u] = ok ? w.dsc[rows[u]] : 0.0;
#pragma unroll
    for (int l = 0; l < PB; ++l) lr[u][l] = 0.0;
  }
  __syncthreads();
  int piv = permL[ps];
  double dpiv = w.dsc[piv];
  // H_k[piv][row] for the next step, loaded as soon as the pivot is known
  double hv[RPT];
#pragma unroll
  for (int u = 0; u < RPT; ++u) hv[u] = w.Hk[size_t(piv) * n + min(rows[u], n - 1)];
  for (int i = ps; i < pe; ++i) {
    const int t = i - ps;
    const double ljj = sqrt(fmax(dpiv, 0.0));
    const double inv = ljj > 0.0 ? 1.0 / ljj : 0.0;
    double bv = -INFINITY;
    int bp = n, bu = -1;
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
      const int r = rows[u];
      if (r >= n) continue;
      if (r == piv) {  // the pivot row itself
#pragma unroll
        for (int l = 0; l < PB; ++l)
          if (l == t) lr[u][l] = ljj;
        continue;
      }
      if (posr[u] <= i) continue;
      double v = hv[u];
#pragma unroll
      for (int l = 0; l < PB; ++l) v -= l < t ? lr[u][l] * lrow[l] : 0.0;
      const double lv = v * inv;
#pragma unroll
      for (int l = 0; l < PB; ++l)
        if (l == t) lr[u][l] = lv;
      dsr[u] -= lv * lv;
      if (dsr[u] > bv || (dsr[u] == bv && posr[u] < bp)) {
        bv = dsr[u];
        bp = posr[u];
        bu = u;
      }
    }
    if (i + 1 >= k) break;  // dgeqp3 stops after k steps: no swap into position k
    // workgroup candidate (largest diagonal, first dgeqp3 position); each
    // wave's winning lane stages its row and L row in LDS
    int bw = tid;
    wave_argmax(bv, bp, bw);
    if (lane == 0) {
      sv[wid] = bv;
      spos[wid] = bp;
      swin[wid] = bw;
    }
    if (tid == bw && bu >= 0) {
#pragma unroll
      for (int u = 0; u < RPT; ++u)
        if (u == bu) {
          wrow[wid][0] = double(rows[u]);
#pragma unroll
          for (int l = 0; l < PB; ++l) wrow[wid][1 + l] = lr[u][l];
        }
    }
    __syncthreads();
    int wq = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (sv[q] > sv[wq] || (sv[q] == sv[wq] && spos[q] < spos[wq])) wq = q;
    // publish: value, position, row, the row's L panel (slot parity = step parity)
    double *mine = w.pp + (size_t(i & 1) * PGMAX + me) * PPS;
    if (wid == 0) {  // one parallel store: [0] value, [1] position, [2] row, [8 + l] L row
      if (lane < 3) mine[lane] = lane == 0 ? sv[wq] : (lane == 1 ? double(spos[wq]) : wrow[wq][0]);
      else if (lane >= 8 && lane - 8 <= t) mine[lane] = wrow[wq][lane - 7];
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    // all-to-all: wait for every workgroup's candidate of this step
    // wave 0 as a whole wave (scalar loop, spin.h): arrive, bounded poll; a
    // stall sets flag[15] and ends every later wait of the launch at once
    if (__builtin_amdgcn_readfirstlane(wid) == 0) {
      tg::wave_arrive(w.cnt);
      const unsigned target = base + unsigned(G) * unsigned(t + 1);
      s_me = tg::spin_geq(w.cnt, target, w.flag + 15, 200000000ull) ? 0 : -1;
    }
    __syncthreads();
    if (s_me < 0) return;
    // every workgroup's record (value, position, row, L row) in one round of
    // parallel sc1 loads, so the winner's L row needs no second round trip
    const double *slots = w.pp + size_t(i & 1) * PGMAX * PPS;
    {
      const int nrec = G * PPS;
      double tmp[PGMAX * PPS / 256];
#pragma unroll
      for (int u = 0; u < PGMAX * PPS / 256; ++u) {
        const int x = tid + u * 256;
        tmp[u] = x < nrec ? ld1(slots + x) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < PGMAX * PPS / 256; ++u) {
        const int x = tid + u * 256;
        if (x < nrec) slotc[x] = tmp[u];
      }
    }
    __syncthreads();
    if (wid == 0) {
      double v = -INFINITY;
      int p2 = n, g = lane;
      if (lane < G) {
        v = slotc[lane * PPS];
        p2 = int(slotc[lane * PPS + 1]);
      }
      wave_argmax(v, p2, g);
      if (lane == 0) {
        s_best = v;
        s_g = g;
        spos[0] = p2;
      }
    }
    __syncthreads();
    const int g = min(max(s_g, 0), G - 1), q = min(max(spos[0], i + 1), n - 1);
    const double *win = slotc + g * PPS;
    if (tid <= t) lrow[tid] = win[8 + tid];
    const int rowb = min(max(int(win[2]), 0), n - 1);
#pragma unroll
    for (int u = 0; u < RPT; ++u) hv[u] = w.Hk[size_t(rowb) * n + min(rows[u], n - 1)];
    const int a = permL[i + 1];
    __syncthreads();
    if (tid == 0 && q != i + 1) {  // dgeqp3 swap of positions i+1 and q (every copy)
      permL[i + 1] = rowb;
      permL[q] = a;
      if (me == 0) {
        w.perm[i + 1] = rowb;
        w.perm[q] = a;
        w.pos[rowb] = i + 1;
        w.pos[a] = q;
      }
    }
#pragma unroll
    for (int u = 0; u < RPT; ++u) {
      if (rows[u] == rowb) posr[u] = i + 1;
      else if (rows[u] == a && q != i + 1) posr[u] = q;
    }
    dpiv = s_best;
    piv = rowb;
    __syncthreads();
  }
  // the panel's L columns, once: row-contiguous into L, coalesced into LT
  const int pw = min(pe, k) - ps;
#pragma unroll
  for (int u = 0; u < RPT; ++u) {
    const int r = rows[u];
    if (r >= n) continue;
    w.dsc[r] = dsr[u];
#pragma unroll
    for (int l = 0; l < PB; ++l) {
      if (l < pw) {
        w.L[size_t(r) * k + ps + l] = lr[u][l];
        w.LT[size_t(l) * n + r] = lr[u][l];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Candidate-set pivoting: one workgroup picks a whole panel's pivots.
//
// Schur diagonals only decrease.  At the start of a panel the rows with the
// (about) SEL largest diagonals form the candidate set C; every other
// unpivoted row stays <= tau = max of their diagonals at panel start.  Step
// 0 of the panel is a full argmax.  At a later step, if the best candidate
// (diagonal desc, dgeqp3 position asc) is strictly above tau it is the exact
// dgeqp3 choice; otherwise the panel ends there (fewer than PB steps) and the
// next panel re-selects.  Only candidates carry their panel of L (one per
// thread, in registers), so a step costs one H_k load and two workgroup
// barriers instead of an all-to-all across workgroups.  piv_fill_kernel then
// computes the panel's L columns and diagonals of ALL rows with the same
// operation sequence (explicit fma), so candidates and the rest agree bit
// for bit.  Selection: two 11-bit radix passes on the diagonal's bit pattern
// (positive doubles order like their bits), set = rows strictly above the
// crossing bin (|set| <= the level's count).
// Levels.  The tau rule gives dgeqp3's choice at any candidate count; the
// count only trades the cost of a step against the length of a panel.  A
// panel runs at one of three levels: 256 or 512 candidates on four waves (one
// per SIMD; one or two candidates per thread), or 1024 on all eight.  The
// selection always uses the eight waves; below 1024 the upper four leave
// before the steps.  The level is a word of sstate, set by each panel for
// the next (lev_pays, LEV_DOWN at sel_steps' end); TG_PIV_LEVEL forces it.
// Every level runs the same operations on a candidate's lr, dc, ljj and inv,
// so piv_fill_kernel reproduces them bit for bit whatever the level.
// Measured at n = 4096, k = 3058 (profiles/piv/README.md): waves of the
// eight-wave form wait 53% of their cycles and issue 32% (VALU 43% of a
// SIMD's cycles), instruction-cache misses are 0.1% of fetches; a step is
// 1.9 us at 1024 candidates, about 1.5 us at 512 and 1.4 us at 256: three
// quarters of it is a latency chain that fewer lanes do not shorten.  256
// candidates give panels of 22 steps on average there, which costs more in
// extra panels than the shorter steps save, so the adaptive rule spends most
// panels at 512.  Only reasoned: how the waits split into barrier, LDS and
// gather.
// The candidate-set path keeps H_k compacted: at a panel starting at step ps
// the Schur complement of the unpivoted rows is the leading (n - ps)^2 block,
// row / column x holding the row at position ps + x (leading dimension n).
// Each panel's Schur update writes the next compacted block into the other
// buffer (syrk_compact_kernel), so the update touches (n - ps)^2 entries
// instead of n^2 and a pivot's row is contiguous.
constexpr int SEL = 1024;        // candidates
constexpr int SEL_LDS_N = 8192;  // n up to which piv_sel_kernel stages diagonals in LDS

#ifdef TG_SEL_PHASES
__device__ unsigned long long g_selph[16];
#define SELT(i)                                                     \
  {                                                                 \
    const uint64_t tt = __builtin_amdgcn_s_memtime();               \
    if (i > 0 && threadIdx.x == 0) atomicAdd(g_selph + i - 1, tt - selt_last); \
    selt_last = tt;                                                 \
  }
#else
#define SELT(i)
#endif

__device__ inline unsigned long long dkey(double d) {
  return d > 0.0 ? static_cast<unsigned long long>(__double_as_longlong(d)) : 0ull;
}

// The compacted H_k buffers keep only their lower triangle (the Schur update
// writes no mirror): entry (a, b) is read at (max, min).  The first panel's
// H_k is the full matrix, for which that is the same entry.
__device__ __forceinline__ size_t hk_at(int a, int b, int n) {
  return size_t(max(a, b)) * n + min(a, b);
}

// n <= 32768 on this path (compact_pivot), so an entry's index fits 32 bits
__device__ __forceinline__ unsigned hk_at32(int a, int b, int n) {
  return unsigned(max(a, b)) * unsigned(n) + unsigned(min(a, b));
}

constexpr int STH = 512;        // threads of piv_sel_kernel (8 waves)

// Candidate levels: 256 (four waves, one candidate per thread), 512 (four
// waves, two per thread), 1024 (eight waves, two per thread).  The words of
// sstate behind the two step counts hold the adaptive level and the counts
// TG_PIV_STATS prints; piv_init2_kernel zeroes them, so a solve starts at the
// lowest level (that can pay at its size, lev_pays).
constexpr int NLEV = 3;
constexpr int LEV_DOWN = 8;  // panels at a level before the next one tries the level below
enum { SS_LEV = 2, SS_RUN = 3, SS_PANELS = 4, SS_EARLY = 5, SS_ESC = 6, SS_NLEV = 7, SS_NEED = 10 };
static_assert(SS_NLEV + NLEV <= SS_NEED && SS_NEED + NLEV - 1 <= 16, "sstate words");

// Does a narrower level pay for a panel of `rem` unpivoted rows that loses
// `lost` of its PB steps to the tau rule?  The lost steps cost their share of
// one more panel (selection and fill, about 35 us, plus the Schur update,
// about 19 us at the flagship's mean rem^2 = 0.44 * 4096^2, i.e. (rem / 64)^2
// / 94 us); four waves save about 0.45 us a step, 14 us a full panel
// (measured at n = 4096, profiles/piv/README.md).  lost = 1 asks whether the
// level can pay at all at this size.
__device__ __forceinline__ bool lev_pays(int rem, int lost) {
  const int r = rem >> 6, extra_us = 35 + r * r / 94, gain_us = 14;
  return lost * extra_us < PB * gain_us;
}

// What the selection hands to a panel's steps.
struct SelPanel {
  int n, k, ps, pe, nset, bp, brow, bo, lev;
  bool adaptive;
  bool pub;  // a publisher wave stores the step records (streamed fill), not the stepping waves
  double tau, bv;
  const double *dS;
  const int32_t *pS;
  int *permL;
  const int *cand;
  double2 *rec;
  int *reco;
  double *lrow;
  unsigned long long t0;  // TG_SEL_PHASES: the last time stamp
};
template <int NW, int CP>
__device__ __forceinline__ void sel_steps(const SelPanel &sp, PivWs w,
                                          const double *__restrict__ Hc);

// Block argmax of (v desc, p asc) carrying a row id r (positions are
// unique).  Wave stage: the maximum of v alone through six exchange stages
// (v_permlane{32,16}_swap pairs, DPP row mirrors / quad perms) with v_max_f64,
// then the holder found by a ballot; only a tie on v (rare: exhausted
// candidates at -inf) takes the slower min-position pass.  One barrier; the
// NW wave records are merged by every thread with selects.
// v_max_f64 without the operand canonicalisation fmax() adds for values that
// come out of lane exchanges
__device__ inline double vmax_d(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ inline double sel_pair_max(double x, bool half16) {
  const int lo = __double2loint(x), hi = __double2hiint(x);
  if (half16) {
    const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return vmax_d(__hiloint2double(h[0], l[0]), __hiloint2double(h[1], l[1]));
  }
  const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return vmax_d(__hiloint2double(h[0], l[0]), __hiloint2double(h[1], l[1]));
}
template <int CTRL>
__device__ inline double sel_dpp(double x) {
  return __hiloint2double(__builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, false),
                          __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, false));
}
__device__ inline double wave_max_d(double x) {
  x = sel_pair_max(x, false);
  x = sel_pair_max(x, true);
  x = vmax_d(x, sel_dpp<0x140>(x));  // lane ^ 15
  x = vmax_d(x, sel_dpp<0x141>(x));  // lane ^ 7
  x = vmax_d(x, sel_dpp<0x1B>(x));   // lane ^ 3
  return vmax_d(x, sel_dpp<0xB1>(x));  // lane ^ 1
}
template <int S>
__device__ inline int wave_min_stage(int x) {
  return min(x, partner<S>(x));
}
// The merge of the NW wave records behind block_argmax_sel's barrier (the
// publisher wave of a streamed panel runs it too, to follow the steps).
template <int NW>
__device__ inline void sel_merge(double &v, int &p, int &r, int &o, const double2 *rec,
                                 const int *reco) {
  double2 x[NW];
#pragma unroll
  for (int q = 0; q < NW; ++q) x[q] = rec[q];
  v = x[0].x;
#pragma unroll
  for (int q = 1; q < NW; ++q) v = vmax_d(v, x[q].x);
  p = INT_MAX;
  r = 0;
  o = 0;
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    const int op = __double2hiint(x[q].y);
    const bool take = (x[q].x == v) & (op < p);
    p = take ? op : p;
    r = take ? __double2loint(x[q].y) : r;
    o = take ? reco[q] : o;
  }
}
template <int NW>
__device__ inline void block_argmax_sel(double &v, int &p, int &r, int &o, double2 *rec,
                                        int *reco) {
  const double m = wave_max_d(v);
  const bool hold = v == m;
  const unsigned long long b = __ballot(hold);
  int L = __ffsll(static_cast<long long>(b)) - 1;
  // tie on v: smallest position among the holders (uniform branch).  A wave
  // whose candidates are all exhausted (every lane at -inf) skips it: its
  // record cannot win unless every wave's is -inf, and then the panel ends
  if (__popcll(b) > 1 && m != -INFINITY) {
    int pp = hold ? p : INT_MAX;
    pp = wave_min_stage<0>(pp);
    pp = wave_min_stage<1>(pp);
    pp = wave_min_stage<2>(pp);
    pp = wave_min_stage<3>(pp);
    pp = wave_min_stage<4>(pp);
    pp = wave_min_stage<5>(pp);
    L = __ffsll(static_cast<long long>(__ballot(hold & (p == pp)))) - 1;
  }
  const int wp = __builtin_amdgcn_readlane(p, L), wr = __builtin_amdgcn_readlane(r, L);
  const int wo = __builtin_amdgcn_readlane(o, L);
  if ((threadIdx.x & 63) == 0) {
    rec[threadIdx.x >> 6] = make_double2(m, __hiloint2double(wp, wr));
    reco[threadIdx.x >> 6] = wo;
  }
  __syncthreads();
  sel_merge<NW>(v, p, r, o, rec, reco);
}

// Radix-select histograms: 2048 bins padded by one word per 32 (bin b at
// b + b / 32), so the scan's lanes (one 32-bin block each) read conflict-free.
constexpr int HPAD = 2048 + 64;
__device__ inline int hidx(int b) { return b + (b >> 5); }

// Wave-aggregated histogram increment: the exponent bins of one wave's keys
// are few (diagonals of similar scale), so one atomic per distinct bin instead
// of 64 same-address atomics.  Uniform loop over the distinct bins.
__device__ inline void hist_add_agg(unsigned *hist, int bin, bool ok, int lane) {
  unsigned long long pend = __ballot(ok);
  while (pend) {
    const int L = __ffsll(static_cast<long long>(pend)) - 1;
    const int b = __builtin_amdgcn_readlane(bin, L);
    const unsigned long long same = __ballot(ok & (bin == b));
    if (lane == L) atomicAdd(&hist[hidx(b)], unsigned(__popcll(same)));
    pend &= ~same;
  }
}

// Wave 0: crossing bin of the `target`-th largest key (bins scanned top-down;
// lane L holds block 63 - L in registers) and the count strictly above it, to
// out[0..1] (LDS).  Written only when the target is reached.
__device__ inline void hist_scan(const unsigned *hist, int target, int *out) {
  const int lane = threadIdx.x & 63, blk = 63 - lane;
  int c[32];
#pragma unroll
  for (int j = 0; j < 32; ++j) c[j] = int(hist[blk * 33 + 31 - j]);  // bin 32 blk + 31 - j
  int sum = 0;
#pragma unroll
  for (int j = 0; j < 32; ++j) sum += c[j];
  int pre = sum;  // inclusive prefix over lanes (top blocks first)
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(pre, off);
    pre += lane >= off ? o : 0;
  }
  int acc = pre - sum;
  if (acc < target && pre >= target) {
    int cb = 0, cbefore = 0;
    bool found = false;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const bool hit = !found & (acc + c[j] >= target);
      cb = hit ? j : cb;
      cbefore = hit ? acc : cbefore;
      found = found | hit;
      acc += c[j];
    }
    out[0] = blk * 32 + 31 - cb;
    out[1] = cbefore;
  }
}

// The pivot's diagonal entry of L and its reciprocal: one sequence for the
// stepping waves and the publisher wave, so both hold the same bits.
__device__ __forceinline__ void piv_scale(double dpiv, double &ljj, double &inv) {
  ljj = sqrt(fmax(dpiv, 0.0));
  inv = ljj > 0.0 ? 1.0 / ljj : 0.0;
}

// ---------------------------------------------------------------------------
// Streamed fill (TG_PIV_STREAM, default on).  The fill of step t needs only
// pivot t, so it does not have to wait for the panel's last step: the
// piv_sel_kernel launch carries fill workers next to the selector, and the
// selector's publisher wave hands them each step's record as the steps go.
//
// Record of step t: prow[t] (pivot row), ppoi[t] (its compact index), pq[t]
// (the position it was swapped in from), pinv[t], Lpp[t][0..t] -- the arrays
// piv_fill_kernel reads, so the same bytes serve the net launch below.
// Progress word strm[0] (one 8-byte sc1 store): launch number | panel start |
// flags | records complete.  Hand-off in the write-through form
// (MI355X_MICROARCH.md "Valid forms", row 1): the publisher wave stores a
// record sc1, drains vmcnt(0) and then stores the word sc1; a worker wave
// polls the word sc1 and reads every record byte sc1 after its poll matched.
// The publisher drains one step late (the stores have had a step to land), so
// it reaches the stepping waves' barriers on time; the stepping waves
// themselves store nothing to global memory in a streamed panel.
//
// A worker is one wave owning the 64 rows at panel-start positions ps + 64 c
// ..; it runs piv_fill_kernel's sequence for its rows record by record and
// follows each row through the published swaps (positions i and q).  L goes
// out four steps at a time; when the panel's end is published the worker
// writes LT (column = final position - ps2) and dsc, marks its chunk in fdone
// and counts it in strm[1].  piv_fill_kernel runs after the launch as a net:
// it returns at once when every chunk is counted, and otherwise fills exactly
// the rows whose panel-start chunk is not marked (L entries a worker that gave
// up had written are rewritten with the same values), so the results never
// depend on co-residency or timing.  One worker per chunk, at most one per
// CU besides the selector's: chunks beyond that are the net's.  Waits: the selector
// never waits for a worker; a worker's polls are bounded by `budget` ticks of
// the 100 MHz clock since its start, after which it leaves without writing
// (budget 0: at once).  A worker reads perm and dsc of its rows before the
// selector's tail rewrites perm: the publisher stores the end of the panel
// and drains before the tail's barrier, and a worker that finds the end
// already published after loading its rows leaves them to the net.
typedef __attribute__((address_space(1))) double pv_f64;
typedef __attribute__((address_space(1))) int32_t pv_i32;
typedef __attribute__((address_space(1))) unsigned long long pv_u64;
__device__ __forceinline__ void st_sc1d(double *p, double v) {
  __hip_atomic_store((pv_f64 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_sc1d(const double *p) {
  return __hip_atomic_load((pv_f64 *)const_cast<double *>(p), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1i(int32_t *p, int v) {
  __hip_atomic_store((pv_i32 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_sc1i(const int32_t *p) {
  return __hip_atomic_load((pv_i32 *)const_cast<int32_t *>(p), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1u(unsigned long long *p, unsigned long long v) {
  __hip_atomic_store((pv_u64 *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long ld_sc1u(const unsigned long long *p) {
  return __hip_atomic_load((pv_u64 *)const_cast<unsigned long long *>(p), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// progress word: [63:32] launch number (> 0), [31:16] panel start, [7] not
// streamed, [6] panel ended, [5:0] step records complete (0 .. PB)
constexpr unsigned long long SW_ENDED = 64ull, SW_NOSTREAM = 128ull, SW_STEPS = 63ull;
static_assert(PB <= int(SW_STEPS), "step count field");
__device__ __forceinline__ unsigned long long sw_word(unsigned seq, int ps) {
  return (static_cast<unsigned long long>(seq) << 32) |
         (static_cast<unsigned long long>(ps & 0xffff) << 16);
}

// Publisher wave of a streamed panel (wave 4 of the selector; NW stepping
// waves).  It joins every barrier of sel_steps<NW, *> -- per step the block
// argmax's (t > 0) and the hand-off's, then the tail's two -- and between them
// stores the step's record from what the stepping waves left in LDS (the
// merged argmax records, the pivot's L row).
template <int NW>
__device__ __forceinline__ void sel_publish(const SelPanel &sp, PivWs w, unsigned seq) {
  const int lane = threadIdx.x & 63;
  const int ps = sp.ps, pe = sp.pe;
  const unsigned long long base = sw_word(seq, ps);
  int piv = sp.brow, q = sp.bp, opiv = sp.bo;
  double dpiv = sp.bv;
  int tdone = 0;
  for (int t = 0; t < PB; ++t) {  // every exit is wave-uniform
    if (ps + t >= pe) break;
    if (t > 0) {
      __syncthreads();  // block_argmax_sel's
      double v;
      int p, r, o;
      sel_merge<NW>(v, p, r, o, sp.rec, sp.reco);
      v = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                           __builtin_amdgcn_readfirstlane(__double2loint(v)));
      // record t - 1 was stored a step ago: drained by now, publish it
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) st_sc1u(w.strm, base | static_cast<unsigned long long>(t));
      if (!(v > sp.tau)) break;
      dpiv = v;
      q = __builtin_amdgcn_readfirstlane(p);
      piv = __builtin_amdgcn_readfirstlane(r);
      opiv = __builtin_amdgcn_readfirstlane(o);
    }
    __syncthreads();  // the step's hand-off: lrow holds the pivot's L row
    double ljj, inv;
    piv_scale(dpiv, ljj, inv);
    if (lane <= t) st_sc1d(w.Lpp + t * PB + lane, lane < t ? sp.lrow[lane] : ljj);
    if (lane == 0) {
      st_sc1i(w.prow + t, piv);
      st_sc1i(w.ppoi + t, opiv);
      st_sc1i(w.pq + t, q);
      st_sc1d(w.pinv + t, inv);
    }
    tdone = t + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (lane == 0) st_sc1u(w.strm, base | SW_ENDED | static_cast<unsigned long long>(tdone));
  __syncthreads();  // the tail's first barrier
  // the end is visible before the tail rewrites perm / pos (behind its second barrier)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// Worker's LDS (the launch's dynamic region): the records.
constexpr int WK_ROWS = 64;
constexpr size_t WK_LDS = sizeof(double) * (PB * PB + PB) + sizeof(int) * 3 * PB;

// Bounded poll of the progress word by a whole wave: until the launch's word
// shows more than `have` records or the panel's end.  0 = budget spent.
__device__ inline unsigned long long strm_wait(const unsigned long long *word, unsigned seq,
                                               int have, uint64_t t0, unsigned budget) {
  unsigned long long v;
  for (;;) {
    const unsigned long long x = ld_sc1u(word);
    v = (static_cast<unsigned long long>(
             __builtin_amdgcn_readfirstlane(static_cast<unsigned>(x >> 32)))
         << 32) |
        __builtin_amdgcn_readfirstlane(static_cast<unsigned>(x));
    if (static_cast<unsigned>(v >> 32) == seq &&
        ((v & (SW_ENDED | SW_NOSTREAM)) != 0ull || int(v & SW_STEPS) > have))
      break;
    if (__builtin_amdgcn_s_memrealtime() - t0 > budget) {
      v = 0ull;
      break;
    }
    __builtin_amdgcn_s_sleep(4);
  }
  // no load of the caller moves above the poll (the record loads are sc1)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return v;
}

// One wave (workgroup blockIdx.x >= 1 of the piv_sel_kernel launch).
__device__ __forceinline__ void piv_stream_worker(int n, int k, PivWs w,
                                                  const double *__restrict__ Hc, unsigned seq,
                                                  unsigned budget, char *smem) {
  double *lpl = reinterpret_cast<double *>(smem);        // PB x PB  pivots' L rows
  double *pinv_s = lpl + PB * PB;                        // PB
  int *prow_s = reinterpret_cast<int *>(pinv_s + PB);    // PB
  int *poi_s = prow_s + PB, *pq_s = poi_s + PB;          // PB each
  const int lane = threadIdx.x, c = int(blockIdx.x) - 1;
  if (seq == 0u || budget == 0u) return;
  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  const unsigned long long hdr = strm_wait(w.strm, seq, -1, t0, budget);
  if (hdr == 0ull || (hdr & SW_NOSTREAM) != 0ull) return;
  const int ps = int((hdr >> 16) & 0xffffull);
  if (ps + WK_ROWS * c >= n) return;
  const int x0 = ps + WK_ROWS * c + lane;
  const bool valid = x0 < n;
  const int xc = valid ? x0 : n - 1;
  const int rl = w.perm[xc];
  const int r = valid ? rl : -1;  // -1: no pivot's row
  const int oi = xc - ps;         // compact index in the panel's H_k (in range also when !valid)
  double d = w.dsc[rl];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  {  // the rows above are the panel-start ones only if the panel has not ended since
    const unsigned long long x = ld_sc1u(w.strm);
    const bool stale = static_cast<unsigned>(x >> 32) != seq || (x & SW_ENDED) != 0ull;
    if (__builtin_amdgcn_readfirstlane(int(stale))) return;
  }
  double lr[PB];
#pragma unroll
  for (int l = 0; l < PB; ++l) lr[l] = 0.0;
  bool done = false;
  int pos = x0;
  int have = 0;
  for (;;) {
    const unsigned long long pw = strm_wait(w.strm, seq, have, t0, budget);
    if (pw == 0ull) return;  // budget spent: nothing written, the net fills the chunk
    const int s = min(int(pw & SW_STEPS), PB);
    if (s > have) {
      // records have .. s - 1 to LDS
      if (lane >= have && lane < s) {
        const int pr = ld_sc1i(w.prow + lane), po = ld_sc1i(w.ppoi + lane), pq = ld_sc1i(w.pq + lane);
        const double pi = ld_sc1d(w.pinv + lane);
        prow_s[lane] = pr;
        poi_s[lane] = min(max(po, 0), n - ps - 1);
        pq_s[lane] = pq;
        pinv_s[lane] = pi;
      }
      for (int e0 = have * PB; e0 < s * PB; e0 += 4 * 64) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int e = e0 + lane + 64 * u;
          v[u] = e < s * PB ? ld_sc1d(w.Lpp + e) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int e = e0 + lane + 64 * u;
          if (e < s * PB) lpl[e] = v[u];
        }
      }
      __syncthreads();  // one live wave: orders the LDS writes before the reads below
      // the new steps' entries of the pivots' rows, all in flight together;
      // lr[j] holds the gathered H_k entry until step j turns it into L
#pragma unroll
      for (int j = 0; j < PB; ++j)
        if (j >= have && j < s) lr[j] = Hc[hk_at(poi_s[j], oi, n)];
      // piv_fill_kernel's sequence, step by step
#pragma unroll
      for (int t = 0; t < PB; ++t) {
        if (t >= have && t < s) {  // uniform
          const double *lp = lpl + t * PB;
          double v = lr[t];
#pragma unroll
          for (int l = 0; l < t; ++l) v = fma(-lr[l], lp[l], v);
          const double lv = v * pinv_s[t];
          const bool act = !done, isp = prow_s[t] == r;
          lr[t] = act ? (isp ? lp[t] : lv) : 0.0;
          d = (act & !isp) ? fma(-lv, lv, d) : d;
          // dgeqp3's swap of positions i and q: the pivot to i, the row at i to q
          const int i = ps + t, q = pq_s[t];
          pos = (act & isp) ? i : ((pos == i) & (q != i)) ? q : pos;
          done = done | (act & isp);
          // L (row-major by row id) goes out four steps at a time while the
          // selector steps on, so the panel's end has only LT and dsc left
          if ((t & 3) == 3 && valid) {
            double *dst = w.L + size_t(r) * k + ps + (t - 3);
#pragma unroll
            for (int u = 0; u < 4; ++u) dst[u] = lr[t - 3 + u];
          }
        }
      }
      have = s;
    }
    if ((pw & SW_ENDED) != 0ull) break;
  }
  const int tn = have, ps2 = ps + tn;
  if (tn <= 0) return;
  if (valid) w.dsc[r] = d;
#pragma unroll
  for (int l = 0; l < PB; ++l) {
    if (valid && pos >= ps2 && pos < n) w.LT[size_t(l) * n + (pos - ps2)] = lr[l];
    if (valid && l >= (tn & ~3) && l < tn) w.L[size_t(r) * k + ps + l] = lr[l];  // the last 0 .. 3
  }
  if (lane == 0) {
    w.fdone[c] = int(seq);
    (void)__hip_atomic_fetch_add((pv_u64 *)(w.strm + 1), 1ull, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One panel: candidate selection, then the panel's steps (pivot rows gathered
// from the compacted H_k).
// Workgroup 0 is the selector; with seq != 0 (the streamed fill, TG_PIV_STREAM)
// workgroups 1.. are fill workers (piv_stream_worker), one wave each.
__global__ __launch_bounds__(STH) void piv_sel_kernel(int n, int k, PivWs w,
                                                      const double *__restrict__ Hc, int flev,
                                                      unsigned seq, unsigned budget) {
  extern __shared__ int permL[];  // n: position -> row
  if (blockIdx.x != 0) {  // uniform
    if (threadIdx.x < 64)
      piv_stream_worker(n, k, w, Hc, seq, budget, reinterpret_cast<char *>(permL));
    return;
  }
  __shared__ unsigned hist[HPAD];
  __shared__ int cand[SEL + 1];  // + trash slot for branch-free compaction
  __shared__ double2 rec[STH / 64];
  __shared__ int reco[STH / 64];
  __shared__ double sv[STH / 64];
  __shared__ int scnt[STH / 64];
  __shared__ int sel[4];
  __shared__ double lrow[PB];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int ps = w.sstate[0];
  if (ps >= k) {
    if (tid == 0) {
      w.sstate[1] = 0;
      if (seq != 0u) st_sc1u(w.strm, sw_word(seq, ps) | SW_NOSTREAM | SW_ENDED);
    }
    return;
  }
  const int pe = min(ps + PB, k);
  // this panel's level and its candidate count: flev >= 0 forces the level;
  // a panel whose Schur update is so large that losing a single step costs
  // more than four waves save keeps the widest
  const int lev = flev >= 0              ? flev
                  : !lev_pays(n - ps, 1) ? NLEV - 1
                                         : min(max(w.sstate[SS_LEV], 0), NLEV - 1);
  const int nsel = SEL >> (NLEV - 1 - lev);
  // streamed fill: below the widest level wave 4 stays on through the steps as
  // the publisher.  The panel's header goes out now (one store, no wait), so
  // the workers load their rows while the candidates are selected; a panel at
  // the widest level steps on all eight waves and is not streamed.
  const bool pub = seq != 0u && lev < NLEV - 1;
  // strm[1] counts the chunks the workers complete (the net launch returns at
  // once when that is all of them); zeroed by the publisher's wave, whose
  // drains put the zero ahead of the end it publishes and so of every add
  if (seq != 0u && tid == 4 * 64) {
    st_sc1u(w.strm + 1, 0ull);
    st_sc1u(w.strm, sw_word(seq, ps) | (pub ? 0ull : SW_NOSTREAM | SW_ENDED));
  }
#ifdef TG_SEL_PHASES
  uint64_t selt_last = 0;
#endif
  SELT(0)
  int nset, bp, brow, bo;
  double tau, bv;
  const double *dS;
  const int32_t *pS;
  // Schur diagonals and positions: staged in LDS once for n <= SEL_LDS_N (the
  // selection passes below read them three times), else read from HBM/L2
  const bool staged = n <= SEL_LDS_N;
  double *dsh = reinterpret_cast<double *>(permL + ((n + 1) & ~1));
  int *posh = reinterpret_cast<int *>(dsh + n);
  if (staged) {
    for (int r0 = tid; r0 < n; r0 += 8 * STH) {
      double dv[8];
      int pv[8], mv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {  // one batch of loads in flight
        const int r = min(r0 + u * STH, n - 1);
        dv[u] = w.dsc[r];
        pv[u] = w.pos[r];
        mv[u] = w.perm[r];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (r0 + u * STH < n) {
          dsh[r0 + u * STH] = dv[u];
          posh[r0 + u * STH] = pv[u];
          permL[r0 + u * STH] = mv[u];
        }
    }
  } else {
    for (int x = tid; x < n; x += STH) permL[x] = w.perm[x];
  }
  for (int x = tid; x < HPAD; x += STH) hist[x] = 0u;
  if (tid == 0) {
    sel[0] = -1;  // b1 (-1: every positive key is a candidate)
    sel[2] = -1;  // b2
  }
  __syncthreads();
  SELT(9)
  dS = staged ? dsh : w.dsc;
  pS = staged ? posh : w.pos;
  // --- candidate set ---------------------------------------------------------
  // one sweep: count of unpivoted rows with positive keys + exponent histogram
  int valid = 0;
  for (int r0 = tid; r0 < n; r0 += 8 * STH) {
    double dv[8];
    int pv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = min(r0 + u * STH, n - 1);
      dv[u] = dS[r];
      pv[u] = pS[r];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const unsigned long long key = dkey(dv[u]);
      const bool ok = (r0 + u * STH < n) & (pv[u] >= ps) & (key != 0ull);
      valid += ok;
      hist_add_agg(hist, int(key >> 52), ok, lane);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) valid += __shfl_xor(valid, off);
  if (lane == 0) scnt[wid] = valid;
  __syncthreads();
  valid = 0;
#pragma unroll
  for (int q = 0; q < STH / 64; ++q) valid += scnt[q];
  SELT(10)
  if (valid > nsel) {  // uniform
    if (wid == 0) hist_scan(hist, nsel, sel);  // sel[0] = b1, sel[1] = count above
    __syncthreads();
    for (int x = tid; x < HPAD; x += STH) hist[x] = 0u;
    __syncthreads();
    const int b1 = sel[0];
    for (int r0 = tid; r0 < n; r0 += 8 * STH) {
      double dv[8];
      int pv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = min(r0 + u * STH, n - 1);
        dv[u] = dS[r];
        pv[u] = pS[r];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const unsigned long long key = dkey(dv[u]);
        if ((r0 + u * STH < n) & (pv[u] >= ps) & (int(key >> 52) == b1))
          atomicAdd(&hist[hidx(int(key >> 41) & 2047)], 1u);  // mantissa bins: spread
      }
    }
    __syncthreads();
    if (wid == 0) hist_scan(hist, nsel - sel[1], sel + 2);
    __syncthreads();
  }
  SELT(11)
  const int b1 = sel[0], b2 = sel[2];
  // compaction of the set, tau over the rest, full argmax for step 0 (branch-free;
  // membership kept as one bit per row of this thread: n <= 64 STH)
  int mine = 0;
  tau = -INFINITY;
  bv = -INFINITY;
  bp = n;
  brow = 0;
  unsigned long long insm = 0ull;
  for (int r0 = tid, bi = 0; r0 < n; r0 += 8 * STH, bi += 8) {
    double dv[8];
    int pv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int r = min(r0 + u * STH, n - 1);
      dv[u] = dS[r];
      pv[u] = pS[r];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool un = (r0 + u * STH < n) & (pv[u] >= ps);
      const unsigned long long key = dkey(dv[u]);
      const int d1 = int(key >> 52), d2 = int(key >> 41) & 2047;
      const bool ins = un & (key != 0ull) & ((b1 < 0) | (d1 > b1) | ((d1 == b1) & (d2 > b2)));
      mine += ins;
      insm |= static_cast<unsigned long long>(ins) << (bi + u);
      tau = (un & !ins) ? fmax(tau, dv[u]) : tau;
      const bool take = un & ((dv[u] > bv) | ((dv[u] == bv) & (pv[u] < bp)));
      bv = take ? dv[u] : bv;
      bp = take ? pv[u] : bp;
      brow = take ? r0 + u * STH : brow;
    }
  }
  {
    int pre = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(pre, off);
      pre += lane >= off ? o : 0;
    }
    double t2 = tau;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t2 = fmax(t2, __shfl_xor(t2, off));
    __syncthreads();  // scnt reuse
    if (lane == 63) scnt[wid] = pre;
    if (lane == 0) sv[wid] = t2;
    __syncthreads();
    int base = 0;
    tau = -INFINITY;
#pragma unroll
    for (int q = 0; q < STH / 64; ++q) {
      base += q < wid ? scnt[q] : 0;
      tau = fmax(tau, sv[q]);
    }
    int slot = base + pre - mine;
    for (int r0 = tid, bi = 0; r0 < n; r0 += 8 * STH, bi += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const bool ins = (insm >> (bi + u)) & 1ull;
        cand[ins ? slot : SEL] = r0 + u * STH;  // non-members to the trash slot
        slot += ins;
      }
    }
  }
  __syncthreads();
  SELT(12)
  nset = 0;
#pragma unroll
  for (int q = 0; q < STH / 64; ++q) nset += scnt[q];
  bo = bp - ps;  // compact index of the step-0 pivot (positions unchanged so far)
  block_argmax_sel<STH / 64>(bv, bp, brow, bo, rec, reco);
  SelPanel sp{n,   k,  ps, pe,    nset, bp,   brow, bo,   lev,  flev < 0, pub,
              tau, bv, dS, pS,    permL, cand, rec,  reco, lrow,
#ifdef TG_SEL_PHASES
              selt_last
#else
              0
#endif
  };
  if (lev == NLEV - 1) {  // uniform
    sel_steps<STH / 64, 2>(sp, w, Hc);
    return;
  }
  // one wave per SIMD from here on: the other four leave (a workgroup
  // barrier counts the waves that have not ended)
  if (wid >= 4) {
    if (pub && wid == 4) sel_publish<4>(sp, w, seq);
    return;
  }
  if (lev == 1) sel_steps<4, 2>(sp, w, Hc);
  else sel_steps<4, 1>(sp, w, Hc);
}

// The panel's steps on NW waves holding CP candidates per thread (NW * 64 * CP
// >= the level's candidate count), then the panel's bookkeeping: positions,
// compact indices, step counts and the next panel's level.
template <int NW, int CP>
__device__ __forceinline__ void sel_steps(const SelPanel &sp, PivWs w,
                                          const double *__restrict__ Hc) {
  constexpr int NT = NW * 64;
  const int tid = threadIdx.x;
  const int n = sp.n, k = sp.k, ps = sp.ps, pe = sp.pe, nset = sp.nset;
  const double tau = sp.tau;
  const double *dS = sp.dS;
  const int32_t *pS = sp.pS;
  int *permL = sp.permL;
  const int *cand = sp.cand;
  double2 *rec = sp.rec;
  int *reco = sp.reco;
  double *lrow = sp.lrow;
#ifdef TG_SEL_PHASES
  uint64_t selt_last = sp.t0;
#endif
  // the level's run length and the counts, read here so that the panel's end
  // only stores
  const int ss_run = w.sstate[SS_RUN], ss_esc = w.sstate[SS_ESC], ss_panels = w.sstate[SS_PANELS],
            ss_early = w.sstate[SS_EARLY], ss_nlev = w.sstate[SS_NLEV + sp.lev],
            ss_need_up = w.sstate[SS_NEED + min(sp.lev, NLEV - 2)],      // leaving this level upwards
            ss_need_dn = w.sstate[SS_NEED + max(sp.lev - 1, 0)];         // entering the level below
  int rc[CP], posc[CP], oc[CP];
  double dc[CP];
  bool done[CP];
  double lr[CP][PB];
#pragma unroll
  for (int u = 0; u < CP; ++u) {
    const int c = tid + u * NT;
    rc[u] = c < nset ? cand[c] : -1;
    posc[u] = rc[u] >= 0 ? pS[rc[u]] : n;
    oc[u] = rc[u] >= 0 ? posc[u] - ps : 0;  // compact index in this panel's H_k
    dc[u] = rc[u] >= 0 ? dS[rc[u]] : -INFINITY;
    done[u] = rc[u] < 0;
#pragma unroll
    for (int l = 0; l < PB; ++l) lr[u][l] = 0.0;
  }
  int piv = sp.brow, q = sp.bp, opiv = sp.bo;
  double dpiv = sp.bv;
  int tdone = 0;
  SELT(1)
  // steps unrolled: the panel column t is a compile-time register index
  bool active = true;  // uniform
  // one instantiation per panel column t: lr[u][t] is a static register index
  auto step = [&]<int t>(std::integral_constant<int, t>) __attribute__((always_inline)) {
    const int i = ps + t;
    active = active && i < pe;
    if (!active) return;
    if (t > 0) {  // candidate argmax; exact only above tau
      double v = -INFINITY;
      int p = n, r = -1, o = 0;
#pragma unroll
      for (int u = 0; u < CP; ++u) {
        const bool take = !done[u] & ((dc[u] > v) | ((dc[u] == v) & (posc[u] < p)));
        v = take ? dc[u] : v;
        p = take ? posc[u] : p;
        r = take ? rc[u] : r;
        o = take ? oc[u] : o;
      }
      SELT(4)
      block_argmax_sel<NW>(v, p, r, o, rec, reco);
      SELT(5)
      active = v > tau;
      if (!active) return;
      dpiv = v;
      q = p;
      piv = r;
      opiv = o;
    }
    double hv[CP];
#pragma unroll
    for (int u = 0; u < CP; ++u)  // H_k[piv][candidate], issued before the hand-off
      hv[u] = Hc[hk_at32(opiv, oc[u], n)];  // unconditional; masked below
#pragma unroll
    for (int u = 0; u < CP; ++u)
      if (rc[u] == piv) {
#pragma unroll
        for (int l = 0; l < t; ++l) lrow[l] = lr[u][l];
      }
    if (tid == 0) {
      const int a = permL[i];
      if (q != i) {
        permL[i] = piv;
        permL[q] = a;
      }
      if (!sp.pub) w.prow[t] = piv;
    }
    SELT(2)
    __syncthreads();
    SELT(3)
    // the pivot's sqrt / reciprocal after the barrier: their latency overlaps
    // the update's fma chains below, which need inv only at their end
    double ljj, inv;
    piv_scale(dpiv, ljj, inv);
    if (!sp.pub) {  // uniform; a streamed panel's publisher wave stores the record
      if (tid == 0) w.pinv[t] = inv;
      if (tid <= t) w.Lpp[t * PB + tid] = tid < t ? lrow[tid] : ljj;
    }
    double lrw[PB > 1 ? PB : 1];
#pragma unroll
    for (int l = 0; l < t; ++l) lrw[l] = lrow[l];
#pragma unroll
    for (int u = 0; u < CP; ++u) {  // branch-free: every slot computes, selects keep
      const bool isp = rc[u] == piv;  // the pivot: dgeqp3 swap of positions i and q
      const bool upd = !done[u] & !isp;
      double v = hv[u];
#pragma unroll
      for (int l = 0; l < t; ++l) v = fma(-lr[u][l], lrw[l], v);
      const double lv = v * inv;
      lr[u][t] = isp ? ljj : (upd ? lv : lr[u][t]);
      dc[u] = upd ? fma(-lv, lv, dc[u]) : dc[u];
      const int pswap = ((posc[u] == i) & (q != i)) ? q : posc[u];
      posc[u] = isp ? i : (upd ? pswap : posc[u]);
      done[u] = done[u] | isp;
    }
    tdone = t + 1;
#ifdef TG_SEL_PHASES
    if (tid == 0) atomicAdd(g_selph + 15, 1ull);
#endif
  };
  [&]<int... Ts>(std::integer_sequence<int, Ts...>) __attribute__((always_inline)) {
    (step(std::integral_constant<int, Ts>{}), ...);
  }(std::make_integer_sequence<int, PB>{});
  SELT(6)
  __syncthreads();
  // compact index (in this panel's H_k) of the row now at position x >= ps:
  // read from the panel-start positions before they are overwritten
  for (int x = ps + tid; x < n; x += NT) w.oidx[x - ps] = pS[permL[x]] - ps;
  __syncthreads();
  for (int x = tid; x < n; x += NT) {
    const int r = permL[x];
    w.perm[x] = r;
    w.pos[r] = x;
  }
  if (tid == 0) {
    w.sstate[0] = ps + tdone;
    w.sstate[1] = tdone;
    // ended by the tau rule: the candidates ran out against the bound of the rest
    const bool early = tdone < PB && ps + tdone < k;
    if (sp.adaptive) {
      // up at once when the tau rule cuts a panel short by more than the
      // narrower level saves (lev_pays: an end one or two steps early costs
      // less than the wider level's steps unless the Schur update is large),
      // down one after `need` panels in a row without such an end.  need
      // starts at LEV_DOWN and doubles, for the rest of the solve, with every
      // raise out of the level below, so a level that keeps failing is
      // retried ever more rarely.
      const bool shorted = early && !lev_pays(n - ps, pe - ps - tdone);
      int lev = sp.lev, run = shorted ? 0 : ss_run + 1;
      if (shorted && lev < NLEV - 1) {
        w.sstate[SS_NEED + lev] = min(2 * max(ss_need_up, LEV_DOWN), 1 << 20);
        ++lev;
        w.sstate[SS_ESC] = ss_esc + 1;
      } else if (lev > 0 && run >= max(ss_need_dn, LEV_DOWN)) {
        --lev;
        run = 0;
      }
      w.sstate[SS_LEV] = lev;
      w.sstate[SS_RUN] = run;
    }
    w.sstate[SS_PANELS] = ss_panels + 1;
    w.sstate[SS_EARLY] = ss_early + early;
    w.sstate[SS_NLEV + sp.lev] = ss_nlev + 1;
  }
}

// The last panel's L columns (L row-major by row; LT panel column-major by
// the NEXT panel's compact index) and Schur diagonals of every row still
// unpivoted at the panel start, with piv_sel_kernel's operation sequence.
// One thread per position x >= ps (row perm[x], compact index oidx[x - ps]
// in the panel's H_k block Hc); rows pivoted in the panel (x < ps + tn) get
// their L entries and no LT column.
// seq != 0: the net behind a streamed panel (launch number seq).  A row whose
// panel-start chunk (compact index / 64) a worker has marked is filled
// already; the kernel fills the others, and a block with none returns.
template <int FT>
__global__ __launch_bounds__(FT) void piv_fill_kernel(int n, int k, PivWs w,
                                                      const double *__restrict__ Hc,
                                                      unsigned seq) {
  __shared__ double lpp[PB][PB + 1];
  __shared__ double pinv[PB];
  __shared__ int prow[PB], poi[PB];
  __shared__ double lst[FT][PB + 1];  // the block's L rows, for row-contiguous stores
  __shared__ int rst[FT];
  const int tid = threadIdx.x;
  const int tn = w.sstate[1];
  const unsigned long long wdone = seq != 0u ? w.strm[1] : 0ull;
  if (tn <= 0) return;
  const int ps = w.sstate[0] - tn, ps2 = ps + tn;
  if (seq != 0u && wdone == static_cast<unsigned long long>(tg::cdiv(n - ps, 64))) return;
  const int x = ps + blockIdx.x * FT + tid;
  const bool valid = x < n;  // no early exit: the L rows go out through LDS below
  const int xc = valid ? x : n - 1;
  const int r = w.perm[xc], oi = w.oidx[xc - ps];
  bool todo = valid;
  if (seq != 0u) {  // uniform
    todo = valid && unsigned(w.fdone[oi >> 6]) != seq;
    if (!__syncthreads_or(todo)) return;
  }
  for (int e = tid; e < PB * PB; e += FT) {
    const int i = e / PB, l = e % PB;
    lpp[i][l] = (i < tn && l <= i) ? w.Lpp[e] : 0.0;
  }
  if (tid < PB) {
    pinv[tid] = tid < tn ? w.pinv[tid] : 0.0;
    prow[tid] = tid < tn ? w.prow[tid] : -1;
    poi[tid] = tid < tn ? w.oidx[tid] : 0;  // pivot i sits at position ps + i
  }
  __syncthreads();
  double hv[PB];
#pragma unroll
  for (int i = 0; i < PB; ++i) hv[i] = i < tn ? Hc[hk_at(poi[i], oi, n)] : 0.0;
  double d = w.dsc[r];
  double lr[PB];
  bool done = false;
  // branch-free (selects, no exec-mask regions around each step, so the
  // broadcast LDS reads of row i of the pivots' L are not serialised behind
  // per-step waits): an inactive step (past the panel's steps, or after this
  // row was pivoted) keeps lr = 0 and d, and its fma terms with lr = 0 leave
  // the later sums unchanged -- the same values as the branchy loop
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    double v = hv[i];
#pragma unroll
    for (int l = 0; l < i; ++l) v = fma(-lr[l], lpp[i][l], v);
    const double lv = v * pinv[i];
    const bool act = (i < tn) & !done, isp = prow[i] == r;
    lr[i] = act ? (isp ? lpp[i][i] : lv) : 0.0;
    d = (act & !isp) ? fma(-lv, lv, d) : d;
    done = done | (act & isp);
  }
  if (todo) w.dsc[r] = d;
#pragma unroll
  for (int l = 0; l < PB; ++l) {
    if (todo && x >= ps2) w.LT[size_t(l) * n + (x - ps2)] = lr[l];
    lst[tid][l] = lr[l];
  }
  rst[tid] = todo ? r : -1;
  __syncthreads();
  // L is row-major by row id (rows scattered): 32 lanes write one row's
  // panel segment contiguously instead of every lane striding k apart
  const int hw = tid >> 5, l = tid & 31;
  for (int t = hw; t < FT; t += FT / 32) {
    const int rr = rst[t];
    if (rr >= 0 && l < tn) w.L[size_t(rr) * k + ps + l] = lst[t][l];
  }
}

typedef double doublex4 __attribute__((ext_vector_type(4)));

// Next panel's compacted H_k: Hn[i][j] = Hc[oidx[tn + i]][oidx[tn + j]]
// - sum_l LT[l][i] LT[l][j] for n - ps2 > i >= j (ps2 = steps done after the
// panel, tn its steps) on 64 x 64 lower tiles: the lower triangle only (8
// bytes per entry of the block read and written instead of 12 with the
// mirror; every reader takes (max, min), hk_at).  The entries are the values
// the mirrored form wrote, bit for bit (a diagonal tile's (a, b) and (b, a)
// are the same products summed in the same order).  The grid covers the
// whole n x n lower triangle; tiles past the block exit.
__global__ __launch_bounds__(256) void syrk_compact_kernel(int n, PivWs w,
                                                           const double *__restrict__ Hc,
                                                           double *__restrict__ Hn) {
  __shared__ double li[PB][64], lj[PB][64];
  __shared__ int orow[64], ocol[64];
  const int tid = threadIdx.x;
  const int ps2 = w.sstate[0], tn = max(w.sstate[1], 0);
  const int nc = n - ps2;
  const int b = blockIdx.x;
  int I = int((sqrt(8.0 * b + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= b) ++I;
  while (I * (I + 1) / 2 > b) --I;
  const int J = b - I * (I + 1) / 2;
  const int i0 = 64 * I, j0 = 64 * J;
  if (i0 >= nc) return;
  if (tid < 64) {
    orow[tid] = w.oidx[tn + min(i0 + tid, nc - 1)];
  } else if (tid < 128) {
    ocol[tid - 64] = w.oidx[tn + min(j0 + tid - 64, nc - 1)];
  }
  for (int e = tid; e < PB * 64; e += 256) {
    const int l = e >> 6, c = e & 63;
    li[l][c] = w.LT[size_t(l) * n + min(i0 + c, nc - 1)];
    lj[l][c] = w.LT[size_t(l) * n + min(j0 + c, nc - 1)];
  }
  __syncthreads();
  // rank-PB update on FP64 MFMA: waves 2 x 2 over the tile, 2 x 2 blocks of
  // 16 x 16 each; the accumulators start from the gathered old values
  const int lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
  const int lr = lane & 15, lk = lane >> 4;
  doublex4 acc[2][2];
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc[ib][jb][q] = Hc[hk_at(orow[wm * 32 + ib * 16 + lk + 4 * q], ocol[wn * 32 + jb * 16 + lr], n)];
#pragma unroll
  for (int kq = 0; kq < PB; kq += 4) {
    double af[2], bf[2];
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) af[ib] = -li[kq + lk][wm * 32 + ib * 16 + lr];
#pragma unroll
    for (int jb = 0; jb < 2; ++jb) bf[jb] = lj[kq + lk][wn * 32 + jb * 16 + lr];
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
        acc[ib][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ib], bf[jb], acc[ib][jb], 0, 0, 0);
  }
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int rl = wm * 32 + ib * 16 + lk + 4 * q, cl = wn * 32 + jb * 16 + lr;
        const int gi = i0 + rl, gj = j0 + cl;
        if (gi < nc && gj < nc && gi >= gj) Hn[size_t(gi) * n + gj] = acc[ib][jb][q];
      }
}

// Persistent form of syrk_compact_kernel (the default): two workgroups per
// CU loop over the tiles of the leading (n - ps2)^2 block (its size read on
// the device); the next tile's gathered old values are loaded while this
// tile is multiplied and written (its row / column indices one step earlier
// still), so the memory pipe does not idle through each workgroup's MFMA,
// epilogue and dispatch.  Same arithmetic per entry as syrk_compact_kernel.
__global__ __launch_bounds__(256, 2) void syrk_compact_p_kernel(int n, PivWs w,
                                                                const double *__restrict__ Hc,
                                                                double *__restrict__ Hn) {
  __shared__ double li[PB][64], lj[PB][64];
  const int tid = threadIdx.x;
  const int ps2 = w.sstate[0], tn = max(w.sstate[1], 0);
  const int nc = n - ps2;
  if (nc <= 0) return;
  const int ntile = tg::cdiv(nc, 64), tiles = ntile * (ntile + 1) / 2;
  const int lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
  const int lr = lane & 15, lk = lane >> 4;
  auto tile_ij = [&](int b, int &i0, int &j0) __attribute__((always_inline)) {
    int I = int((sqrt(8.0 * b + 1.0) - 1.0) * 0.5);
    while ((I + 1) * (I + 2) / 2 <= b) ++I;
    while (I * (I + 1) / 2 > b) --I;
    i0 = 64 * I;
    j0 = 64 * (b - I * (I + 1) / 2);
  };
  // this thread's gathered rows (ib, q) and columns (jb) of a tile
  auto load_idx = [&](int b, int (&ro)[2][4], int (&co)[2]) __attribute__((always_inline)) {
    int i0, j0;
    tile_ij(b, i0, j0);
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int q = 0; q < 4; ++q) ro[ib][q] = w.oidx[tn + min(i0 + wm * 32 + ib * 16 + lk + 4 * q, nc - 1)];
#pragma unroll
    for (int jb = 0; jb < 2; ++jb) co[jb] = w.oidx[tn + min(j0 + wn * 32 + jb * 16 + lr, nc - 1)];
  };
  auto load_old = [&](const int (&ro)[2][4], const int (&co)[2], double (&o)[2][2][4])
      __attribute__((always_inline)) {
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int q = 0; q < 4; ++q) o[ib][jb][q] = Hc[hk_at(ro[ib][q], co[jb], n)];
  };
  int b = blockIdx.x;
  if (b >= tiles) return;
  int ro[2][4], co[2];
  double old[2][2][4], nold[2][2][4];
  load_idx(b, ro, co);
  load_old(ro, co, old);
  const int G = int(gridDim.x);
  if (b + G < tiles) load_idx(b + G, ro, co);
  for (; b < tiles; b += G) {
    int i0, j0;
    tile_ij(b, i0, j0);
    __syncthreads();  // the previous tile's reads of li, lj are done
    double lv[8][2];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = tid + u * 256, l = e >> 6, c = e & 63;
      lv[u][0] = w.LT[size_t(l) * n + min(i0 + c, nc - 1)];
      lv[u][1] = w.LT[size_t(l) * n + min(j0 + c, nc - 1)];
    }
    __builtin_amdgcn_sched_barrier(0);
    const bool more = b + G < tiles;
    if (more) load_old(ro, co, nold);  // in flight through this tile
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = tid + u * 256, l = e >> 6, c = e & 63;
      li[l][c] = lv[u][0];
      lj[l][c] = lv[u][1];
    }
    __syncthreads();
    if (b + 2 * G < tiles) load_idx(b + 2 * G, ro, co);
    doublex4 acc[2][2];
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[ib][jb][q] = old[ib][jb][q];
#pragma unroll
    for (int kq = 0; kq < PB; kq += 4) {
      double af[2], bf[2];
#pragma unroll
      for (int ib = 0; ib < 2; ++ib) af[ib] = -li[kq + lk][wm * 32 + ib * 16 + lr];
#pragma unroll
      for (int jb = 0; jb < 2; ++jb) bf[jb] = lj[kq + lk][wn * 32 + jb * 16 + lr];
#pragma unroll
      for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
          acc[ib][jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ib], bf[jb], acc[ib][jb], 0, 0, 0);
    }
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int rl = wm * 32 + ib * 16 + lk + 4 * q, cl = wn * 32 + jb * 16 + lr;
          const int gi = i0 + rl, gj = j0 + cl;
          if (gi < nc && gj < nc && gi >= gj) Hn[size_t(gi) * n + gj] = acc[ib][jb][q];
        }
#pragma unroll
    for (int ib = 0; ib < 2; ++ib)
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int q = 0; q < 4; ++q) old[ib][jb][q] = nold[ib][jb][q];
  }
}

// dsc = diag(Hk), perm = pos = identity, no pivot chosen yet.
__global__ __launch_bounds__(256) void piv_init2_kernel(int n, PivWs w) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    w.dsc[j] = w.Hk[size_t(j) * n + j];
    w.perm[j] = j;
    w.pos[j] = j;
    if (j < tg::cdiv(n, 64)) w.fdone[j] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) w.strm[threadIdx.x] = 0ull;
  if (blockIdx.x == 0 && threadIdx.x < 16) w.sstate[threadIdx.x] = 0;
}

// Rx[t][j] = L[perm[j]][t] for j >= t (upper trapezoidal), perm64 = perm.
__global__ void rx_gather_kernel(int n, int k, PivWs w, double *__restrict__ Rx, int ldr,
                                 int64_t *__restrict__ perm64) {
  const int t = blockIdx.y;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    const int r = w.perm[j];
    if (t == 0) perm64[j] = r;
    if (Rx) Rx[size_t(t) * ldr + j] = j >= t ? w.L[size_t(r) * k + t] : 0.0;
  }
}

}  // namespace

extern "C" size_t tg_pivot_workspace_size(int n, int k) {
  tg::Sizer s;
  piv_layout(s, n, k, nullptr);
  return s.off + 256;
}

// Greedy diagonal pivoting on w.Hk (filled by the caller) -> perm, R_x.
// Candidate-set pivot order (piv_sel_kernel + piv_fill_kernel per panel).
// Panels end early when the candidate bound fails, so the host launches the
// panels full panels would need, reads the step count once, and continues
// while steps remain.  The Schur update of a round's last panel is issued
// only once more steps are known to follow.
static int pivot_core_sel(hipStream_t st, PivWs &w, int n, int k) {
#ifdef TG_SEL_PHASES
  static bool reg = false;
  if (!reg) {
    reg = true;
    atexit([] {
      unsigned long long h[16];
      (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_selph), sizeof(h));
      const char *nm[12] = {"sel:argmax+cand", "head", "barrier2", "compute+wargmax", "blockargmax",
                            "?", "tail", "?", "sel:stage", "sel:count", "sel:radix", "sel:compact"};
      fprintf(stderr, "sel phases (cycles, thread 0):");
      for (int q = 0; q < 12; ++q) fprintf(stderr, " %s %.3g", nm[q], double(h[q]));
      fprintf(stderr, " steps %llu", h[15]);
      fprintf(stderr, "\n");
    });
  }
#endif
  hipLaunchKernelGGL(piv_init2_kernel, dim3(std::min(64, tg::cdiv(n, 256))), dim3(256), 0, st, n, w);
  TG_LAUNCHED();
  // TG_PIV_STREAM=0: the fill as a launch of its own behind the steps
  // (development switch, per call).  TG_PIV_STREAM_BUDGET: the workers' wait
  // budget in ticks of the 100 MHz clock (default 2 ms; 0: every worker
  // leaves at once and the net launch fills everything)
  const char *sv = getenv("TG_PIV_STREAM");
  const bool stream = !(sv && sv[0] == '0');
  unsigned budget = 200000u;
  if (const char *sb = getenv("TG_PIV_STREAM_BUDGET")) budget = unsigned(strtoul(sb, nullptr, 10));
  unsigned seq = 0;  // launch number of a streamed panel (0: not streamed)
  const size_t lds = std::max(sizeof(int) * size_t((n + 1) & ~1) +
                                  (n <= SEL_LDS_N ? (sizeof(double) + sizeof(int)) * size_t(n) : 0),
                              stream ? WK_LDS : size_t(0));
  if (lds > 48 * 1024)
    TG_HIP(hipFuncSetAttribute((const void *)piv_sel_kernel,
                               hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
  // TG_SYR2K_PERSIST=0: one tile per workgroup (development switch, per call)
  const char *ps = getenv("TG_SYR2K_PERSIST");
  const bool persist = !(ps && ps[0] == '0');
  const tg::XcdInfo xi = tg::xcd_info();
  const int ncu = std::max(1, xi.xcds * xi.cus_per_xcd);
  // compacted Schur complements alternate between the two buffers
  const double *hc = w.Hk;
  double *hn = w.Hk2;
  auto schur_compact = [&](int rows) -> hipError_t {
    const int nt = tg::cdiv(rows, 64);
    if (persist)
      hipLaunchKernelGGL(syrk_compact_p_kernel, dim3(std::min(nt * (nt + 1) / 2, 2 * ncu)),
                         dim3(256), 0, st, n, w, hc, hn);
    else
      hipLaunchKernelGGL(syrk_compact_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, st, n, w, hc,
                         hn);
    const hipError_t e = hipGetLastError();
    double *t = const_cast<double *>(hc);
    hc = hn;
    hn = t;
    return e;
  };
  // TG_PIV_LEVEL=256|512|1024 forces the candidate level of every panel
  // (development switch, per call); unset: chosen on the device, panel by panel
  int flev = -1;
  if (const char *pl = getenv("TG_PIV_LEVEL")) {
    const int v = atoi(pl);
    flev = v == 256 ? 0 : v == 512 ? 1 : v == 1024 ? 2 : -1;
  }
  int done = 0;
  // a panel's Schur update runs at the head of the next panel
  int pend_rows = 0;  // rows of the pending update (0: none)
  for (int round = 0;; ++round) {
    if (round > 4 * (k / PB + 2)) {
      tg::set_error("pivot order: no progress after %d rounds (%d of %d steps)", round, done, k);
      return int(hipErrorUnknown);
    }
    const int P = tg::cdiv(k - done, PB);
    // every panel starts at or after `done + p` steps: grids sized for that bound
    for (int p = 0; p < P; ++p) {
      const int rows = n - (done + p);
      if (pend_rows > 0) TG_HIP(schur_compact(pend_rows));
      auto tok = tg::prof_begin(st, tg::PROF_PIVSTEP, 8.0 * double(n) * PB * 3, 0.0);
      // streamed: one worker per 64-row chunk, at most one per remaining CU
      // (chunks beyond that are the net launch's)
      const int nwork = stream ? std::min(ncu - 1, tg::cdiv(rows, WK_ROWS)) : 0;
      if (stream) ++seq;
      hipLaunchKernelGGL(piv_sel_kernel, dim3(1 + nwork), dim3(STH), lds, st, n, k, w, hc, flev, seq,
                         budget);
      // one wave per workgroup: the gathers of the pivots' columns spread
      // over 4x the CUs of 256-thread groups (n = 12,288: -1.4 ms per solve)
      hipLaunchKernelGGL(piv_fill_kernel<64>, dim3(tg::cdiv(rows, 64)), dim3(64), 0, st, n, k, w, hc,
                         seq);
      tg::prof_end(st, tok);
      TG_LAUNCHED();
      pend_rows = rows;
    }
    int32_t h = 0;
    TG_HIP(hipMemcpyAsync(&h, w.sstate, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    if (h >= k) break;
    pend_rows = n - (done + P - 1);  // the round's last panel, updated at the next one's head
    done = h;
  }
  // TG_PIV_STATS=1: one line per call (development switch)
  if (const char *pst = getenv("TG_PIV_STATS"); pst && pst[0] == '1') {
    int32_t h[16];
    TG_HIP(hipMemcpyAsync(h, w.sstate, sizeof(h), hipMemcpyDeviceToHost, st));
    TG_HIP(hipStreamSynchronize(st));
    fprintf(stderr,
            "pivot stats: n=%d k=%d panels=%d early=%d escalations=%d level256=%d level512=%d "
            "level1024=%d\n",
            n, k, h[SS_PANELS], h[SS_EARLY], h[SS_ESC], h[SS_NLEV], h[SS_NLEV + 1], h[SS_NLEV + 2]);
  }
  return 0;
}

static int pivot_core(hipStream_t st, PivWs &w, int n, int k, int64_t *perm, double *Rx, int ldr) {
  if (compact_pivot(n)) {
    const int e = pivot_core_sel(st, w, n, k);
    if (e != 0) return e;
    hipLaunchKernelGGL(rx_gather_kernel, dim3(tg::cdiv(n, 256) < 16 ? tg::cdiv(n, 256) : 16, k),
                       dim3(256), 0, st, n, k, w, Rx, ldr, perm);
    TG_LAUNCHED();
    return 0;
  }
  const int g0 = std::min(PGMAX, tg::cdiv(n, 256));
  hipLaunchKernelGGL(piv_init_kernel, dim3(g0), dim3(256), 0, st, n, w);
  TG_LAUNCHED();
  const int G = std::max(1, std::min(PGMAX, tg::cdiv(n, 256)));
  const int rpt = tg::cdiv(n, G * 256);
  const bool persistent = rpt <= 2 && n <= 32768 && getenv("TG_PIVOT_STEPWISE") == nullptr;
  if (persistent && n * sizeof(int) > 64 * 1024) {
    TG_HIP(hipFuncSetAttribute((const void *)piv_panel_kernel<1>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, int(n * sizeof(int))));
    TG_HIP(hipFuncSetAttribute((const void *)piv_panel_kernel<2>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, int(n * sizeof(int))));
  }
  TG_HIP(hipMemsetAsync(w.flag, 0, 16 * sizeof(unsigned), st));
  // the arrival counter of the panel kernels starts at 0 after piv_init
  for (int ps = 0; ps < k; ps += PB) {
    const int pe = std::min(ps + PB, k);
    if (persistent) {
      // per-panel: n rows x (PB/2 + 3) doubles of H row, L panel and diagonal
      auto tok = tg::prof_begin(st, tg::PROF_PIVSTEP, 8.0 * double(n) * (pe - ps) * 3, 0.0);
      const size_t lds = sizeof(int) * size_t(n);
      TG_HIP(hipMemsetAsync(w.flag + 4, 0, 9 * sizeof(unsigned), st));
      const int grid = 8 * G;  // >= 8 (G - 1) + 1: some XCD always collects G tickets
      if (rpt == 1)
        hipLaunchKernelGGL(piv_panel_kernel<1>, dim3(grid), dim3(256), lds, st, n, k, ps, pe, G,
                           unsigned(G) * unsigned(ps), w);
      else
        hipLaunchKernelGGL(piv_panel_kernel<2>, dim3(grid), dim3(256), lds, st, n, k, ps, pe, G,
                           unsigned(G) * unsigned(ps), w);
      tg::prof_end(st, tok);
      TG_LAUNCHED();
    } else {
      for (int i = ps; i < pe; ++i) {
        auto tok = tg::prof_begin(st, tg::PROF_PIVSTEP, 8.0 * double(n - i) * (i - ps + 3), 0.0);
        hipLaunchKernelGGL(piv_step_kernel, dim3(G), dim3(256), 0, st, n, k, i, ps, w);
        tg::prof_end(st, tok);
        TG_LAUNCHED();
      }
    }
    if (pe < k)  // Schur update with this panel's columns (all rows, original order)
      TG_HIP(tg::dsyrk_tn(st, n, pe - ps, -1.0, w.LT, n, 1.0, w.Hk, n));
  }
  hipLaunchKernelGGL(rx_gather_kernel, dim3(tg::cdiv(n, 256) < 16 ? tg::cdiv(n, 256) : 16, k),
                     dim3(256), 0, st, n, k, w, Rx, ldr, perm);
  TG_LAUNCHED();
  return 0;
}

extern "C" int tg_pivoted_factor(void *stream, const double *Vh, int ldv, const double *S, int n,
                                 int k, int64_t *perm, double *Rx, int ldr, void *ws,
                                 size_t ws_bytes) {
  TG_ARG(Vh, 2, "null Vh");
  TG_ARG(ldv >= n, 3, "ldv < n");
  TG_ARG(S, 4, "null S");
  TG_ARG(n >= 1, 5, "n < 1");
  TG_ARG(k >= 1 && k <= n, 6, "k must be in [1, n]");
  TG_ARG(perm, 7, "null perm");
  TG_ARG(!Rx || ldr >= n, 9, "ldr < n");
  hipStream_t st = (hipStream_t)stream;
  tg::Arena ar(ws, ws_bytes);
  PivWs w{};
  piv_layout(ar, n, k, &w);
  TG_WS(ar);
  TG_HIP(hipMemsetAsync(w.cnt, 0, 16 * sizeof(unsigned), st));
  TG_HIP(hipMemsetAsync(w.LT, 0, sizeof(double) * PB * size_t(n), st));
  hipLaunchKernelGGL(scale_rows_kernel, dim3(tg::cdiv(n, 256) < 16 ? tg::cdiv(n, 256) : 16, k),
                     dim3(256), 0, st, Vh, ldv, S, n, k, w.B);
  TG_LAUNCHED();
  TG_HIP(tg::dsyrk_tn(st, n, k, 1.0, w.B, n, 0.0, w.Hk, n));  // H_k = H_sqrt^T H_sqrt
  return pivot_core(st, w, n, k, perm, Rx, ldr);
}

// Complement form: H_k = H - B_c^T B_c with B_c = diag(S_c) Vc, the nc
// dropped eigenpairs that are not at rounding level (k < j < k + nc in
// descending order).  Equal to V_k L_k V_k^T up to the dropped eigenvalues
// below the rounding threshold; nc may be 0.
extern "C" int tg_pivoted_factor_complement(void *stream, const double *H, int ldh,
                                            const double *Vc, int ldvc, const double *Sc, int nc,
                                            int n, int k, int64_t *perm, double *Rx, int ldr,
                                            void *ws, size_t ws_bytes) {
  TG_ARG(H, 2, "null H");
  TG_ARG(n >= 1, 8, "n < 1");
  TG_ARG(k >= 1 && k <= n, 9, "k must be in [1, n]");
  TG_ARG(ldh >= n, 3, "ldh < n");
  TG_ARG(nc >= 0 && nc <= k && k + nc <= n, 7, "nc must be in [0, min(k, n - k)]");
  TG_ARG(nc == 0 || Vc, 4, "null Vc");
  TG_ARG(nc == 0 || ldvc >= n, 5, "ldvc < n");
  TG_ARG(nc == 0 || Sc, 6, "null Sc");
  TG_ARG(perm, 10, "null perm");
  TG_ARG(!Rx || ldr >= n, 12, "ldr < n");
  hipStream_t st = (hipStream_t)stream;
  tg::Arena ar(ws, ws_bytes);
  PivWs w{};
  piv_layout(ar, n, k, &w);
  TG_WS(ar);
  TG_HIP(hipMemsetAsync(w.cnt, 0, 16 * sizeof(unsigned), st));
  TG_HIP(hipMemsetAsync(w.LT, 0, sizeof(double) * PB * size_t(n), st));
  TG_HIP(hipMemcpy2DAsync(w.Hk, sizeof(double) * n, H, sizeof(double) * ldh, sizeof(double) * n,
                          n, hipMemcpyDeviceToDevice, st));
  if (nc > 0) {
    hipLaunchKernelGGL(scale_rows_kernel, dim3(tg::cdiv(n, 256) < 16 ? tg::cdiv(n, 256) : 16, nc),
                       dim3(256), 0, st, Vc, ldvc, Sc, n, nc, w.B);
    TG_LAUNCHED();
    TG_HIP(tg::dsyrk_tn(st, n, nc, -1.0, w.B, n, 1.0, w.Hk, n));
  }
  return pivot_core(st, w, n, k, perm, Rx, ldr);
}
