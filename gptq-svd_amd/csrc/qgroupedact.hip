// A22: grouped packed GEMM with MXFP8 activations -- the expert layer of an
// MXFP4 Mixture-of-Experts model on v_mfma_scale_f32_16x16x128_f8f6f4:
//
//   Y[i, r] = round(row_scale[i] * sum_k X^[rows[i], k] * W^_e[r, k]),
//   offsets[e] <= i < offsets[e + 1],
//
// X^ the MXFP8 image of X that tg_quant_act_mx defines, W^_e expert e's MXFP4
// pair.  The e4m3 bytes and the packed E2M1 words go to the matrix pipe as they
// lie in memory with both E8M0 bytes in a VGPR: no weight is decoded on the
// VALU, there is no LDS in the K loop and no barrier.
//
// The T rows of X are quantised once, row-major (tg_quant_act_mx into the
// workspace): with top-k routing a token feeds k slots, and an image in slot
// order would quantise and store it k times and need the experts' runs padded
// to tile boundaries that only the device knows.  Each lane gathers its rows
// through `rows` instead: two 16-byte loads at row stride n per step.
//
// One kernel for every R.  A workgroup of four waves owns BM slots of one
// expert (find_work, as in qgrouped.hip) x 64 features; BM = 16: the waves side
// by side along the features, one 16 x 16 tile each, odd and even K steps in
// accumulators of their own; BM = 64: 2 x 2 waves of 32 slots x 32 features.  A
// K step is one MFMA depth, 128 values = 4 blocks; four steps' operands are in
// registers at once (the ring of qmxact_kernel).  K is split over blockIdx.z
// while the tiles alone do not fill the device: the fp32 partial tiles go to
// the workspace and qgrouped_reduce_kernel adds them in ascending split order,
// applies row_scale and rounds once.  Decode is this kernel with BM = 16 and
// split K.  No atomics: bit-identical from call to call.
#include <cstdlib>
#include <cstring>

#include "../../include/truncgptq.h"
#include "common.h"
#include "qdtype.h"
#include "qgrouped_work.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int GA_TILE = 64;         // output features per workgroup
constexpr int GA_KS = 128;          // K step: one MFMA depth, 4 blocks of 32
constexpr int GA_TARGET_WGS = 512;  // MA_TARGET_WGS / MA_MIN_STEPS of qmxact.hip
constexpr int GA_MIN_STEPS = 4;
constexpr int GA_SMALL_RUN = 32;    // average run up to which the 16-slot tile is used

// operands of one K step of a wave: MI slot tiles of X^, NJ feature tiles of W^_e
template <int MI, int NJ>
struct Frag {
  u32x4 a[MI][2];   // e4m3 bytes: k = 16 g + [0, 16) and 64 + 16 g + [0, 16), g = lane >> 4
  u32x4 b[NJ];      // packed E2M1 words: k = 32 g + [0, 32)
  uint32_t sa[MI], sb[NJ];
};

// grid: (slot tiles, feature tiles, K splits).  Steps [blockIdx.z * sps, + sps)
// of the K range.  part == nullptr (one split): row_scale and the output
// rounding happen here; otherwise the fp32 tile goes to part[z][R][m] and
// qgrouped_reduce_kernel finishes.
template <int MI, int NJ, int WR, int WC, int NS>
__global__ __launch_bounds__(256) void qgroupedact_kernel(
    const uint8_t *__restrict__ xq, const uint8_t *__restrict__ xs, int T,
    const int32_t *__restrict__ rows, const int32_t *__restrict__ offsets, int R, int E,
    const uint32_t *__restrict__ qw, const uint8_t *__restrict__ sc, int m, int n, int sps,
    float *__restrict__ part, const float *__restrict__ row_scale, void *__restrict__ Y, int y_dt,
    int64_t ldy) {
  static_assert(WR * WC == 4 && NJ * WC * 16 == GA_TILE);
  constexpr int BM = 16 * MI * WR;
  constexpr bool PARITY = MI * NJ == 1;  // one tile a wave: even and odd steps accumulate apart
  static_assert(NS >= 2 && (!PARITY || NS % 2 == 0));
  const Work wk = find_work(offsets, E, R, BM, blockIdx.x);
  if (wk.e < 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave / WC, wc = wave % WC;
  const int lr = lane & 15, g = lane >> 4;
  const int slot0 = wk.s0 + wr * MI * 16, col0 = blockIdx.y * GA_TILE + wc * NJ * 16;
  const int units = n / 32;
  const int steps = tg::cdiv(n, GA_KS);
  const int s0 = blockIdx.z * sps, s1 = min(steps, s0 + sps);

  // expert e's pair inside the stacked tensors
  const uint32_t *qe = qw + int64_t(wk.e) * (n / 8) * m;
  const uint8_t *se = sc + int64_t(wk.e) * units * m;

  // This lane's A rows, resolved once: the token behind slot slot0 + 16 i + lr.
  // Slots past the run and tokens outside [0, T) (a malformed rows) load
  // nothing, so no index leaves xq or xs.
  const uint8_t *arow[MI];
  const uint8_t *srow[MI];
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int slot = slot0 + i * 16 + lr;
    int token = -1;
    if (slot < wk.s1) token = rows ? rows[slot] : slot;
    const bool ok = token >= 0 && token < T;
    arow[i] = ok ? xq + int64_t(token) * n : nullptr;
    srow[i] = ok ? xs + int64_t(token) * units : nullptr;
  }

  f32x4 acc[MI][NJ], acc2[PARITY ? 1 : MI][PARITY ? 1 : NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (PARITY) acc2[0][0] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Blocks past n (a K tail of one to three blocks inside a step), slots past
  // the run and features past m load nothing: their operands are zero, so they
  // add exactly 0 whatever the scale byte (127 there).
  auto fetch = [&](int s, Frag<MI, NJ> &f) {
    const int u = s * 4 + g;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const bool rv = s < s1 && arow[i] != nullptr;
      const int k = s * GA_KS + 16 * g;
      // n % 32 == 0: a run of 16 bytes never straddles n; token * n is a multiple of 32
      f.a[i][0] = (rv && k < n) ? *reinterpret_cast<const u32x4 *>(arow[i] + k)
                                : u32x4{0u, 0u, 0u, 0u};
      f.a[i][1] = (rv && k + 64 < n) ? *reinterpret_cast<const u32x4 *>(arow[i] + k + 64)
                                     : u32x4{0u, 0u, 0u, 0u};
      f.sa[i] = (rv && u < units) ? uint32_t(srow[i][u]) : 127u;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int o = col0 + j * 16 + lr;
      const bool wv = s < s1 && o < m && u < units;
      f.b[j] = u32x4{0u, 0u, 0u, 0u};
      f.sb[j] = 127u;
      if (wv) {
#pragma unroll
        for (int w = 0; w < 4; ++w) f.b[j][w] = qe[(int64_t(u) * 4 + w) * m + o];
        f.sb[j] = se[int64_t(u) * m + o];
      }
    }
  };

  // cbsz = 0 (A e4m3), blgp = 4 (B fp4); operand, scale-lane and C/D layouts as
  // documented at qmxact_kernel's mma (qmxact.hip).
  auto mma = [&](const Frag<MI, NJ> &f, f32x4 (&c)[MI][NJ]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const i32x8 av = {int(f.a[i][0][0]), int(f.a[i][0][1]), int(f.a[i][0][2]),
                          int(f.a[i][0][3]), int(f.a[i][1][0]), int(f.a[i][1][1]),
                          int(f.a[i][1][2]), int(f.a[i][1][3])};
        const i32x8 bv = {int(f.b[j][0]), int(f.b[j][1]), int(f.b[j][2]), int(f.b[j][3]),
                          0, 0, 0, 0};
        c[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            av, bv, c[i][j], 0, 4, 0, int(f.sa[i]), 0, int(f.sb[j]));
      }
  };

  // the ring of NS steps' operands: the loads of step s + NS - 1 are issued
  // before the MFMAs of step s
  Frag<MI, NJ> f[NS];
#pragma unroll
  for (int i = 0; i < NS - 1; ++i) fetch(s0 + i, f[i]);
  for (int s = s0; s < s1; s += NS) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      fetch(s + i + NS - 1, f[(i + NS - 1) % NS]);
      if (s + i < s1) mma(f[i], (PARITY && (i & 1)) ? acc2 : acc);  // NS even: i's parity is the step's
    }
  }
  if constexpr (PARITY) acc[0][0] += acc2[0][0];

  // C/D: col = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int slot = slot0 + i * 16 + 4 * g + e;
      if (slot >= wk.s1) continue;
      const float rs = (row_scale && !part) ? row_scale[slot] : 1.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int col = col0 + j * 16 + lr;
        if (col >= m) continue;
        if (part)
          part[(int64_t(blockIdx.z) * R + slot) * m + col] = acc[i][j][e];
        else
          store_from_float(Y, y_dt, int64_t(slot) * ldy + col,
                           row_scale ? acc[i][j][e] * rs : acc[i][j][e]);
      }
    }
}

// Slots per workgroup, from R and E alone (an expert's run length is on the
// device): 16 while the average run R / E is at most 32 slots, 64 above -- the
// rule of qmxact.hip's act_rows on the average run.  TG_QGROUPED_ACT = 16 | 64
// (read per call) forces a height.
int act_slots(int R, int E) {
  const char *e = getenv("TG_QGROUPED_ACT");
  if (e && strcmp(e, "16") == 0) return 16;
  if (e && strcmp(e, "64") == 0) return 64;
  return int64_t(R) <= int64_t(E) * GA_SMALL_RUN ? 16 : 64;
}

// K steps per workgroup: act_steps_per_split of qmxact.hip on the bound of this
// call's tiles (the true count is on the device): one split once the tiles
// alone fill the device, otherwise enough for ~GA_TARGET_WGS workgroups of at
// least GA_MIN_STEPS steps
int grouped_steps_per_split(int R, int E, int m, int n, int BM) {
  const int nstep = tg::cdiv(n, GA_KS);
  const int64_t tiles = int64_t(tg::cdiv(m, GA_TILE)) * tile_bound(R, E, BM);
  int64_t S = (GA_TARGET_WGS + tiles - 1) / (tiles > 0 ? tiles : 1);
  const int s_max = nstep / GA_MIN_STEPS > 1 ? nstep / GA_MIN_STEPS : 1;
  if (S > s_max) S = s_max;
  if (S < 1) S = 1;
  return tg::cdiv(nstep, S);
}

// the workspace: X^ row-major (T x n bytes, T x n/32 scale bytes), the partial tiles
template <class A>
void layout(A &a, int T, int R, int m, int n, int S, uint8_t *&xq, uint8_t *&xs, float *&part) {
  xq = a.template take_aligned<uint8_t>(size_t(T) * n, 256);
  xs = a.template take_aligned<uint8_t>(size_t(T) * (n / 32), 256);
  part = S > 1 ? a.template take_aligned<float>(size_t(S) * R * m, 256) : nullptr;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" size_t tg_qgemm_grouped_act_workspace_size(int T, int R, int E, int m, int n) {
  if (T <= 0 || R <= 0 || E < 1 || E > GR_MAX_E || m <= 0 || n < 32) return 0;
  const int S = tg::cdiv(tg::cdiv(n, GA_KS), grouped_steps_per_split(R, E, m, n, act_slots(R, E)));
  tg::Sizer sz;
  uint8_t *xq, *xs;
  float *part;
  layout(sz, T, R, m, n, S, xq, xs, part);
  return sz.off;
}

extern "C" int tg_qgemm_grouped_act(void *stream, const void *X, int x_dtype, int T,
                                    int64_t stride_x, const int32_t *rows, const int32_t *offsets,
                                    int R, int E, const int32_t *qweight,
                                    const uint8_t *scales_e8m0, int wfmt, int act_fmt, int m, int n,
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
  TG_ARG(scales_e8m0, 11, "null scales");
  TG_ARG(wfmt == TG_FMT_MXFP4, 12, "wfmt must be TG_FMT_MXFP4");
  TG_ARG(act_fmt == TG_ACT_MXFP8, 13, "act_fmt must be TG_ACT_MXFP8");
  TG_ARG(m > 0, 14, "m <= 0");
  TG_ARG((int64_t(m) * 4) % 32 == 0, 14, "m * 4 must be a multiple of 32");
  TG_ARG(n > 0 && n % 32 == 0, 15, "n must be a positive multiple of 32");
  TG_ARG(stride_x >= n, 5, "stride_x < n");
  TG_ARG(Y, 17, "null Y");
  TG_ARG(y_dtype == x_dtype || y_dtype == TG_F32, 18, "y_dtype must be x_dtype or TG_F32");
  TG_ARG(stride_y >= m, 19, "stride_y < m");
  const int ftiles = tg::cdiv(m, GA_TILE);
  TG_ARG(ftiles <= 65535, 14, "m too large");
  const int BM = act_slots(R, E);
  const int sps = grouped_steps_per_split(R, E, m, n, BM);
  const int S = tg::cdiv(tg::cdiv(n, GA_KS), sps);
  TG_ARG(S <= 65535, 15, "n too large");
  TG_ARG(ws, 20, "null workspace");
  tg::Arena arena(ws, ws_bytes);
  uint8_t *xq, *xs;
  float *part;
  layout(arena, T, R, m, n, S, xq, xs, part);
  TG_WS(arena);
  // each token once, row-major: the quantiser of the ABI (launch_quant<false>)
  const int rc = tg_quant_act_mx(stream, X, x_dtype, T, stride_x, n, TG_ACT_MXFP8, xq, n, xs);
  if (rc != 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(unsigned(tile_bound(R, E, BM)), ftiles, S);
  const uint32_t *qw = reinterpret_cast<const uint32_t *>(qweight);
#define TG_GA(MI_, NJ_, WR_, WC_, NS_)                                                           \
  hipLaunchKernelGGL((qgroupedact_kernel<MI_, NJ_, WR_, WC_, NS_>), grid, dim3(256), 0, st, xq, xs, \
                     T, rows, offsets, R, E, qw, scales_e8m0, m, n, sps, part, row_scale, Y,      \
                     y_dtype, stride_y)
  if (BM == 16) TG_GA(1, 1, 1, 4, 4);
  else TG_GA(2, 2, 2, 2, 4);
#undef TG_GA
  TG_LAUNCHED();
  if (S > 1) {
    hipLaunchKernelGGL(qgrouped_reduce_kernel, dim3(tg::cdiv(int64_t(R) * m, 256)), dim3(256), 0, st,
                       part, S, R, m, row_scale, Y, y_dtype, stride_y);
    TG_LAUNCHED();
  }
  return 0;
}
