// A19: grouped packed GEMM -- the expert layer of a Mixture-of-Experts model.
// E packed matrices (stacked images of the A14 / A15 layouts), each applied to
// its own run of "slots":
//
//   Y[i, r] = round(row_scale[i] * sum_k X[rows[i], k] * W^_e[r, k]),
//   offsets[e] <= i < offsets[e + 1].
//
// offsets (E + 1 int32) and rows (R int32, nullable) live on the device and are
// never read on the host: the grid is sized from R and E alone, and every
// workgroup finds its (expert, slot range) itself (find_work) and leaves when it
// has none.  A workgroup's slots belong to one expert, so it unpacks one
// expert's words, once, into the operand type.
//
// Two regimes (TG_QGROUPED = auto | rows | tiles, read per call):
//  * rows (R <= RW_MAX_R): decode.  A workgroup = 64 output features x 4 waves
//    takes a run of up to RW_RUN slots of one expert; K is split over
//    blockIdx.y and, inside the workgroup, over the waves.  The run's gathered X
//    rows of the K chunk are staged in LDS as fp32 and read as a broadcast; a
//    word row of qweight is read coalesced, each word once per run.  The waves'
//    sums are added in wave order and written as part[s][slot][r]; a second
//    kernel adds the partials in ascending s, multiplies by row_scale and rounds
//    once.  A run of one slot, the common case at decode, takes a body with one
//    accumulator.
//  * tiles (any R): a workgroup owns BM (64 or 128) slots of one expert x 64
//    features.  Per K slab of 128 values the expert's weight tile is unpacked
//    into LDS in the operand type beside the X tile gathered through rows, and
//    each wave runs mfma_f32_16x16x32 on its quarter; the next slab's words and
//    X rows are fetched before the MFMAs of the current one.  No split-K.
// No atomics anywhere: the result is bit-identical from call to call.
#include <cstdlib>
#include <cstring>

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "../../include/truncgptq.h"
#include "common.h"
#include "qdtype.h"
#include "qgrouped_work.h"
#include "qunpack.h"

namespace {

// A decoded weight as operand bits.  The contract's operand is tg_dequant_packed's:
// the fp32 product rounded to fp32, then once more to the operand type.  Left to
// itself the compiler fuses the multiply and the conversion to fp16 into one
// v_fma_mixlo_f16, which rounds the exact product once; the two differ on about
// one weight in 10^5 (measured: DESIGN.md "Grouped packed GEMM").  The empty asm
// keeps the fp32 value out of the fused pattern's reach and costs no instruction
// of its own.
template <int DT>
__device__ inline uint16_t operand_bits(float w) {
  asm("" : "+v"(w));
  return to_bits<DT>(w);
}

// expert e's images inside the stacked tensors
template <int B, int FMT>
struct Expert {
  const uint32_t *qw, *qz;
  const void *sc;
  __device__ Expert(const uint32_t *qw0, const uint32_t *qz0, const void *sc0, int sc_dt, int e,
                    int m, int n, int g) {
    const int64_t nzw = (int64_t(m) * B) >> 5, G = n / g;
    qw = qw0 + int64_t(e) * ((int64_t(n) * B) >> 5) * m;
    if constexpr (FMT == FMT_MX) {
      qz = nullptr;
      sc = static_cast<const uint8_t *>(sc0) + int64_t(e) * (n / 32) * m;
    } else {
      qz = qz0 + int64_t(e) * G * nzw;
      sc = static_cast<const char *>(sc0) + int64_t(e) * G * m * (sc_dt == TG_F32 ? 4 : 2);
    }
  }
};

// ---------------------------------------------------------------------------
// rows regime
// ---------------------------------------------------------------------------
constexpr int RW_FEAT = 64;         // output features per workgroup (one per lane)
constexpr int RW_WAVES = 4;         // K sub-slices of a workgroup
constexpr int RW_RUN = 4;           // slots of one expert a workgroup takes
constexpr int RW_MAX_UNITS = 16;    // K chunk of a workgroup <= 512 values (X in LDS as fp32)
constexpr int RW_MAX_R = 128;       // slots the regime takes
constexpr int RW_AUTO_R = RW_MAX_R; // slots up to which TG_QGROUPED=auto picks it: the bare calls
                                    // cross above the cap (DESIGN.md "Grouped packed GEMM")
constexpr int RW_TARGET_WGS = 1024; // ~4 workgroups per CU of a 256-CU device

// units of 32 values per workgroup along K; the number of K splits follows
int rows_units_per_wg(int R, int E, int m, int n) {
  const int units = n / 32;
  const int64_t wgs = int64_t(tg::cdiv(m, RW_FEAT)) * tile_bound(R, E, RW_RUN);
  int64_t S = (RW_TARGET_WGS + wgs - 1) / (wgs > 0 ? wgs : 1);
  const int s_max = tg::cdiv(units, RW_WAVES), s_min = tg::cdiv(units, RW_MAX_UNITS);
  if (S > s_max) S = s_max;
  if (S < s_min) S = s_min;
  if (S < 1) S = 1;
  return tg::cdiv(units, S);
}

// this wave's units [ua, ue) of the workgroup's chunk against TT rows of xs
template <int B, int DT, int FMT, int TT>
__device__ inline void rows_body(const Expert<B, FMT> &ex, int sc_dt, int m, int g, int rc, int u0,
                                 int ua, int ue, const float (*xs)[RW_MAX_UNITS * 32],
                                 float (&acc)[RW_RUN]) {
  const int64_t nzw = (int64_t(m) * B) >> 5;
  float a[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) a[t] = 0.f;
  int cur = -1, z = 0;
  float s = 0.f;
  for (int u = ua; u < ue; ++u) {
    uint32_t w[B];
#pragma unroll
    for (int j = 0; j < B; ++j) w[j] = ex.qw[(int64_t(u) * B + j) * m + rc];
    if constexpr (FMT == FMT_MX) {  // a unit is a group: its byte, one per lane
      s = mx_half_scale(static_cast<const uint8_t *>(ex.sc)[int64_t(u) * m + rc]);
    } else {
      const int gi = (u * 32) / g;  // g % 32 == 0: a unit lies in one group
      if (gi != cur) {
        cur = gi;
        z = zero_value(ex.qz + int64_t(gi) * nzw, rc, B);
        s = scale_value(ex.sc, sc_dt, int64_t(gi) * m + rc);
      }
    }
    const int kl = (u - u0) * 32;
#pragma unroll
    for (int i4 = 0; i4 < 8; ++i4) {
      float wv[4];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        wv[c] = from_bits<DT>(operand_bits<DT>(unit_weight<B, FMT>(w, i4 * 4 + c, z, s)));
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const float4 x = *reinterpret_cast<const float4 *>(&xs[t][kl + i4 * 4]);
        a[t] = fmaf(x.x, wv[0], a[t]);
        a[t] = fmaf(x.y, wv[1], a[t]);
        a[t] = fmaf(x.z, wv[2], a[t]);
        a[t] = fmaf(x.w, wv[3], a[t]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < RW_RUN; ++t) acc[t] = t < TT ? a[t < TT ? t : 0] : 0.f;
}

// grid: (feature tiles, K splits, runs)
template <int B, int DT, int FMT>
__global__ __launch_bounds__(256, 4) void qgrouped_rows_kernel(
    const uint16_t *__restrict__ X, int T, int64_t ldx, const int32_t *__restrict__ rows,
    const int32_t *__restrict__ offsets, int R, int E, const uint32_t *__restrict__ qw,
    const uint32_t *__restrict__ qz, const void *__restrict__ sc, int sc_dt, int m, int n, int g,
    int ub, float *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) float xs[RW_RUN][RW_MAX_UNITS * 32];
  __shared__ float red[RW_WAVES][RW_RUN][RW_FEAT];
  __shared__ int src[RW_RUN];
  const Work wk = find_work(offsets, E, R, RW_RUN, blockIdx.z);
  if (wk.e < 0) return;
  const int nrow = wk.s1 - wk.s0;  // 1 .. RW_RUN
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < RW_RUN) {
    const int slot = min(wk.s0 + tid, wk.s1 - 1);
    src[tid] = min(max(rows ? rows[slot] : slot, 0), T - 1);
  }
  __syncthreads();
  const int units = n / 32;
  const int u0 = blockIdx.y * ub, u1 = min(units, u0 + ub);
  const int k0 = u0 * 32, len = (u1 - u0) * 32;
  const int nx = nrow == 1 ? 1 : RW_RUN;  // rows of xs the body reads; those past the run are zero
  for (int idx = tid; idx < nx * len; idx += 256) {
    const int t = idx / len, k = idx - t * len;
    xs[t][k] = t < nrow ? from_bits<DT>(X[int64_t(src[t]) * ldx + k0 + k]) : 0.f;
  }
  __syncthreads();

  const int r = blockIdx.x * RW_FEAT + lane;
  const int rc = min(r, m - 1);  // lanes past m read the last feature and write nothing
  const Expert<B, FMT> ex(qw, qz, sc, sc_dt, wk.e, m, n, g);
  const int uw = tg::cdiv(u1 - u0, RW_WAVES);
  const int ua = u0 + wave * uw, ue = min(u1, ua + uw);
  float acc[RW_RUN];
  if (nrow == 1) rows_body<B, DT, FMT, 1>(ex, sc_dt, m, g, rc, u0, ua, ue, xs, acc);
  else rows_body<B, DT, FMT, RW_RUN>(ex, sc_dt, m, g, rc, u0, ua, ue, xs, acc);
#pragma unroll
  for (int t = 0; t < RW_RUN; ++t) red[wave][t][lane] = acc[t];
  __syncthreads();
  for (int idx = tid; idx < nrow * RW_FEAT; idx += 256) {
    const int t = idx >> 6, l = idx & 63;
    const int rr = blockIdx.x * RW_FEAT + l;
    if (rr < m) {
      float v = red[0][t][l];
#pragma unroll
      for (int wv = 1; wv < RW_WAVES; ++wv) v += red[wv][t][l];
      part[(int64_t(blockIdx.y) * R + wk.s0 + t) * m + rr] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// tiles regime
// ---------------------------------------------------------------------------
// slots per workgroup: 128 once the experts average two 64-slot tiles (every
// unpacked weight then feeds twice the MFMAs), 64 below
int tiles_rows(int R, int E) { return int64_t(R) >= int64_t(E) * 128 ? 128 : 64; }

// grid: (row tiles, feature tiles).  Xs / Ws as in qgemm_mfma_kernel: a wave
// owns BM/2 slots x 32 features, the thread of (wave, lane) unpacks unit `wave`
// of each slab for feature col0 + lane.
template <int B, int DT, int BM, int FMT>
__global__ __launch_bounds__(256) void qgrouped_tiles_kernel(
    const uint16_t *__restrict__ X, int T, int64_t ldx, int xvec, const int32_t *__restrict__ rows,
    const int32_t *__restrict__ offsets, int R, int E, const uint32_t *__restrict__ qw,
    const uint32_t *__restrict__ qz, const void *__restrict__ sc, int sc_dt, int m, int n, int g,
    const float *__restrict__ row_scale, void *__restrict__ Y, int y_dt, int64_t ldy) {
  constexpr int MI = BM / 32;   // 16-row MFMA tiles per wave
  constexpr int XV = BM / 16;   // 8-element groups of the X tile per thread
  __shared__ __attribute__((aligned(16))) uint16_t Xs[BM][MF_LD];
  __shared__ __attribute__((aligned(16))) uint16_t Ws[MF_TILE][MF_LD];
  const Work wk = find_work(offsets, E, R, BM, blockIdx.x);
  if (wk.e < 0) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int col0 = blockIdx.y * MF_TILE;
  const int units = n / 32;
  const int64_t nzw = (int64_t(m) * B) >> 5;
  const int r = col0 + lane;
  const Expert<B, FMT> ex(qw, qz, sc, sc_dt, wk.e, m, n, g);
  // the X rows behind this thread's groups of the tile (-1: past the run)
  int xrow[XV];
#pragma unroll
  for (int i = 0; i < XV; ++i) {
    const int slot = wk.s0 + ((tid + 256 * i) >> 4);
    xrow[i] = slot < wk.s1 ? min(max(rows ? rows[slot] : slot, 0), T - 1) : -1;
  }
  f32x4 acc[MI][2];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // registers of the slab in flight
  uint32_t w[B];
  u32x4 xr[XV];
  bool wvalid = false;
  int cur = -1, z = 0;
  float s = 0.f;
  auto fetch = [&](int ks) {
    const int u = ks / 32 + wave;
    wvalid = r < m && u < units;
    if (wvalid) {
#pragma unroll
      for (int j = 0; j < B; ++j) w[j] = ex.qw[(int64_t(u) * B + j) * m + r];
      if constexpr (FMT == FMT_MX) {
        s = mx_half_scale(static_cast<const uint8_t *>(ex.sc)[int64_t(u) * m + r]);
      } else {
        const int gi = (u * 32) / g;  // g % 32 == 0: a unit lies in one group
        if (gi != cur) {
          cur = gi;
          z = zero_value(ex.qz + int64_t(gi) * nzw, r, B);
          s = scale_value(ex.sc, sc_dt, int64_t(gi) * m + r);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < B; ++j) w[j] = 0u;
    }
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      const int gk = ks + ((tid + 256 * i) & 15) * 8;
      xr[i] = u32x4{0u, 0u, 0u, 0u};
      if (xrow[i] >= 0 && gk < n) {  // n % 8 == 0: a group of 8 never straddles n
        const uint16_t *p = X + int64_t(xrow[i]) * ldx + gk;
        if (xvec) {
          xr[i] = *reinterpret_cast<const u32x4 *>(p);
        } else {
          xr[i] = u32x4{uint32_t(p[0]) | (uint32_t(p[1]) << 16),
                        uint32_t(p[2]) | (uint32_t(p[3]) << 16),
                        uint32_t(p[4]) | (uint32_t(p[5]) << 16),
                        uint32_t(p[6]) | (uint32_t(p[7]) << 16)};
        }
      }
    }
  };

  fetch(0);
  for (int ks = 0; ks < n; ks += MF_KS) {
    // weight tile: Ws[feature][k] = W^_e[col0 + feature][ks + k]
    {
      uint32_t pk[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t lo = operand_bits<DT>(unit_weight<B, FMT>(w, 2 * i, z, s));
        const uint32_t hi = operand_bits<DT>(unit_weight<B, FMT>(w, 2 * i + 1, z, s));
        pk[i] = wvalid ? (lo | (hi << 16)) : 0u;
      }
      u32x4 *dst = reinterpret_cast<u32x4 *>(&Ws[lane][wave * 32]);
#pragma unroll
      for (int i = 0; i < 4; ++i) dst[i] = u32x4{pk[4 * i], pk[4 * i + 1], pk[4 * i + 2], pk[4 * i + 3]};
    }
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      const int v = tid + 256 * i;
      *reinterpret_cast<u32x4 *>(&Xs[v >> 4][(v & 15) * 8]) = xr[i];
    }
    __syncthreads();
    if (ks + MF_KS < n) fetch(ks + MF_KS);
    // lane l: A[row l & 15][k = 8 (l >> 4) + j], B[k = 8 (l >> 4) + j][col l & 15]
#pragma unroll
    for (int kk = 0; kk < MF_KS / 32; ++kk) {
      const int ko = kk * 32 + 8 * (lane >> 4);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = mfma16<DT>(&Xs[wr * (BM / 2) + i * 16 + (lane & 15)][ko],
                                 &Ws[wc * 32 + j * 16 + (lane & 15)][ko], acc[i][j]);
    }
    __syncthreads();
  }
  // C/D: col = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int slot = wk.s0 + wr * (BM / 2) + i * 16 + 4 * (lane >> 4) + e;
      if (slot >= wk.s1) continue;
      const float rs = row_scale ? row_scale[slot] : 1.f;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = col0 + wc * 32 + j * 16 + (lane & 15);
        if (col < m)
          store_from_float(Y, y_dt, int64_t(slot) * ldy + col,
                           row_scale ? acc[i][j][e] * rs : acc[i][j][e]);
      }
    }
}

// ---- host dispatch ----------------------------------------------------------
struct Call {
  hipStream_t st;
  const uint16_t *X;
  int x_dt, T;
  int64_t ldx;
  const int32_t *rows, *offsets;
  int R, E;
  const uint32_t *qw, *qz;
  const void *sc;
  int sc_dt, m, n, g;
  const float *row_scale;
  void *Y;
  int y_dt;
  int64_t ldy;
};

template <int B, int FMT>
void launch_rows(const Call &c, dim3 grid, int ub, float *part) {
#define TG_RW(DT_)                                                                             \
  hipLaunchKernelGGL((qgrouped_rows_kernel<B, DT_, FMT>), grid, dim3(256), 0, c.st, c.X, c.T, c.ldx, \
                     c.rows, c.offsets, c.R, c.E, c.qw, c.qz, c.sc, c.sc_dt, c.m, c.n, c.g, ub, part)
  if (c.x_dt == TG_F16) TG_RW(TG_F16);
  else TG_RW(TG_BF16);
#undef TG_RW
}

template <int B, int FMT>
void launch_tiles(const Call &c, dim3 grid, int BM, int xvec) {
#define TG_TL(DT_, BM_)                                                                         \
  hipLaunchKernelGGL((qgrouped_tiles_kernel<B, DT_, BM_, FMT>), grid, dim3(256), 0, c.st, c.X, c.T, \
                     c.ldx, xvec, c.rows, c.offsets, c.R, c.E, c.qw, c.qz, c.sc, c.sc_dt, c.m, c.n, \
                     c.g, c.row_scale, c.Y, c.y_dt, c.ldy)
  if (c.x_dt == TG_F16) {
    if (BM == 128) TG_TL(TG_F16, 128);
    else TG_TL(TG_F16, 64);
  } else {
    if (BM == 128) TG_TL(TG_BF16, 128);
    else TG_TL(TG_BF16, 64);
  }
#undef TG_TL
}

// TG_QGROUPED (read per call): 0 auto (rows up to R = 128, tiles above), 1 rows (R <= 128), 2 tiles
int qgrouped_mode() {
  const char *e = getenv("TG_QGROUPED");
  if (e && strcmp(e, "rows") == 0) return 1;
  if (e && strcmp(e, "tiles") == 0) return 2;
  return 0;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" size_t tg_qgemm_grouped_workspace_size(int R, int E, int m, int n) {
  if (R <= 0 || R > RW_MAX_R || E < 1 || E > GR_MAX_E || m <= 0 || n < 32) return 0;
  const int S = tg::cdiv(n / 32, rows_units_per_wg(R, E, m, n));
  return size_t(S) * size_t(R) * size_t(m) * sizeof(float) + 256;
}

extern "C" int tg_qgemm_grouped(void *stream, const void *X, int x_dtype, int T, int64_t stride_x,
                                const int32_t *rows, const int32_t *offsets, int R, int E,
                                const int32_t *qweight, const int32_t *qzeros, const void *scales,
                                int scale_dtype, int wfmt, int m, int n, int group, int w_bits,
                                const float *row_scale, void *Y, int y_dtype, int64_t stride_y,
                                void *ws, size_t ws_bytes) {
  TG_ARG(R >= 0, 8, "R < 0");
  if (R == 0) return 0;
  TG_ARG(X, 2, "null X");
  TG_ARG(x_dtype == TG_F16 || x_dtype == TG_BF16, 3, "x_dtype must be TG_F16 or TG_BF16");
  TG_ARG(T > 0, 4, "T <= 0");
  TG_ARG(rows || T == R, 4, "rows is null: slot i reads row i, so T must be R");
  TG_ARG(offsets, 7, "null offsets");
  TG_ARG(E >= 1 && E <= GR_MAX_E, 9, "E must be in [1, 256]");
  TG_ARG(qweight, 10, "null qweight");
  TG_ARG(scales, 12, "null scales");
  TG_ARG(wfmt == 0 || wfmt == TG_FMT_MXFP4, 14, "wfmt must be 0 (integer) or TG_FMT_MXFP4");
  TG_ARG(m > 0, 15, "m <= 0");
  TG_ARG(n > 0 && n % 32 == 0, 16, "n must be a positive multiple of 32");
  TG_ARG(stride_x >= n, 5, "stride_x < n");
  int g = 32;
  if (wfmt == TG_FMT_MXFP4) {
    TG_ARG(group == 32, 17, "MXFP4 has group 32");
    TG_ARG(w_bits == 4, 18, "MXFP4 has w_bits 4");
  } else {
    TG_ARG(qzeros, 11, "null qzeros");
    TG_ARG(scale_dtype == TG_F16 || scale_dtype == TG_F32, 13,
           "scale_dtype must be TG_F16 or TG_F32");
    TG_ARG(bits_ok(w_bits), 18, "w_bits must be 2, 3, 4 or 8");
    g = group > 0 ? group : n;
    TG_ARG(g % 32 == 0 && n % g == 0, 17, "group must be a multiple of 32 that divides n");
  }
  TG_ARG((int64_t(m) * w_bits) % 32 == 0, 15, "m * w_bits must be a multiple of 32");
  TG_ARG(Y, 20, "null Y");
  TG_ARG(y_dtype == x_dtype || y_dtype == TG_F32, 21, "y_dtype must be x_dtype or TG_F32");
  TG_ARG(stride_y >= m, 22, "stride_y < m");
  const int mode = qgrouped_mode();
  TG_ARG(!(mode == 1 && R > RW_MAX_R), 8, "TG_QGROUPED=rows takes R <= 128");
  const bool use_rows = mode == 1 || (mode == 0 && R <= RW_AUTO_R);
  const int ftiles = tg::cdiv(m, MF_TILE);
  TG_ARG(ftiles <= 65535, 15, "m too large");

  const Call c{(hipStream_t)stream, static_cast<const uint16_t *>(X), x_dtype, T, stride_x, rows,
               offsets, R, E, reinterpret_cast<const uint32_t *>(qweight),
               reinterpret_cast<const uint32_t *>(qzeros), scales, scale_dtype, m, n, g, row_scale,
               Y, y_dtype, stride_y};
  const bool mx = wfmt == TG_FMT_MXFP4;

  if (use_rows) {
    const int ub = rows_units_per_wg(R, E, m, n);
    const int S = tg::cdiv(n / 32, ub);
    TG_ARG(S <= 65535, 16, "n too large");
    TG_ARG(ws, 23, "null workspace");
    tg::Arena arena(ws, ws_bytes);
    float *part = arena.take_aligned<float>(size_t(S) * R * m, 256);
    TG_WS(arena);
    const dim3 grid(ftiles, S, int(tile_bound(R, E, RW_RUN)));
    if (mx) launch_rows<4, FMT_MX>(c, grid, ub, part);
    else with_bits(w_bits, [&](auto b) { launch_rows<b.value, FMT_INT>(c, grid, ub, part); });
    TG_LAUNCHED();
    hipLaunchKernelGGL(qgrouped_reduce_kernel, dim3(tg::cdiv(int64_t(R) * m, 256)), dim3(256), 0,
                       c.st, part, S, R, m, row_scale, Y, y_dtype, stride_y);
    TG_LAUNCHED();
    return 0;
  }

  const int BM = tiles_rows(R, E);
  const dim3 grid(unsigned(tile_bound(R, E, BM)), ftiles);
  const int xvec = (reinterpret_cast<uintptr_t>(X) % 16 == 0 && stride_x % 8 == 0) ? 1 : 0;
  if (mx) launch_tiles<4, FMT_MX>(c, grid, BM, xvec);
  else with_bits(w_bits, [&](auto b) { launch_tiles<b.value, FMT_INT>(c, grid, BM, xvec); });
  TG_LAUNCHED();
  return 0;
}
