// A17: the two format-agnostic kernels that apply a low-rank correction A B
// beside a packed GEMM (qlinear.hip, qmxact.hip; their device code is unchanged):
//
//   Y32 = X W^^T                      the packed GEMM, fp32 output, no bias
//   Z   = X B^T          (T x r)      tg_lr_down
//   Y   = round(Y32 + Z A^T + bias)   tg_lr_finish
//
// Numerics (fixed, reproducible on the host): X, B and A are converted exactly
// to fp32; every product and sum is an fp32 fma; tg_lr_finish starts each
// output from Y32[t, o], adds Z[t, j] A[o, j] in ascending j, then the bias, and
// rounds once to the output type.  No atomics: bit-identical from call to call.
//
// tg_lr_down, two regimes (switch TG_LR_DOWN = auto | gemv | mfma, read per call):
//  * gemv (T <= 16): a wave owns one row of B over the workgroup's K chunk and
//    every row of X; a lane takes 8 consecutive k per pass (one 16-byte load
//    of a 16-bit operand), the lanes' sums meet in a fixed butterfly.
//  * mfma (any T): a workgroup owns 128 rows of X x 32 rows of B; K slabs of 32
//    go through LDS as fp32 into v_mfma_f32_32x32x2_f32 (the exact-fp32 matrix
//    instruction: X and B need not share a 16-bit type, and B may be fp32).
// The output is tiny (T x r), so both regimes split K over blockIdx until about
// LR_TARGET_WGS workgroups run; with S > 1 splits the partial sums [S][T][r] go
// to the workspace and qgemv_reduce_kernel adds them in ascending split order.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/truncgptq.h"
#include "common.h"
#include "qdtype.h"

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int LR_MAX_RANK = 128;
constexpr int LR_TARGET_WGS = 512;  // ~2 workgroups per CU of a 256-CU device

// TG_LR_TARGET_WGS (development switch, read per call; tools/lrc_bench.py sweeps it)
int target_wgs() {
  const char *e = getenv("TG_LR_TARGET_WGS");
  const int v = e ? atoi(e) : 0;
  return v > 0 ? v : LR_TARGET_WGS;
}

// p[i .. i+8) of dtype dt as fp32 (exact).  vec: the address is 16-byte aligned
__device__ inline void load8(const void *p, int dt, int64_t i, bool vec, float *o) {
  if (dt == TG_F32) {
    const float *s = static_cast<const float *>(p) + i;
    if (vec) {
      const float4 a = *reinterpret_cast<const float4 *>(s);
      const float4 b = *reinterpret_cast<const float4 *>(s + 4);
      o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w;
      o[4] = b.x, o[5] = b.y, o[6] = b.z, o[7] = b.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = s[e];
    }
    return;
  }
  const uint16_t *s = static_cast<const uint16_t *>(p) + i;
  uint32_t w[4];
  if (vec) {
    const u32x4 v = *reinterpret_cast<const u32x4 *>(s);
    w[0] = v[0], w[1] = v[1], w[2] = v[2], w[3] = v[3];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = uint32_t(s[2 * e]) | (uint32_t(s[2 * e + 1]) << 16);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint16_t h = uint16_t(w[e >> 1] >> (16 * (e & 1)));
    o[e] = dt == TG_F16 ? from_bits<TG_F16>(h) : from_bits<TG_BF16>(h);
  }
}

// may 16-byte loads be taken from rows of this matrix at multiples of 8 elements?
bool vec_ok(const void *p, int dt, int64_t ld) {
  const int per16 = dt == TG_F32 ? 4 : 8;
  return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % per16 == 0;
}

// ---------------------------------------------------------------------------
// tg_lr_down, gemv regime
// ---------------------------------------------------------------------------
constexpr int GD_WAVES = 4;     // rows of B per workgroup, one per wave
constexpr int GD_PASS = 512;    // k per pass of a wave: 64 lanes x 8
constexpr int GD_MAX_T = 16;    // rows the gemv regime takes
constexpr int GD_AUTO_T = 16;   // rows up to which TG_LR_DOWN=auto picks it (measured)

// K chunk of a workgroup, a multiple of GD_PASS; the number of splits follows
int gemv_chunk(int r, int n) {
  const int passes = tg::cdiv(n, GD_PASS), tiles = tg::cdiv(r, GD_WAVES);
  int S = tg::cdiv(target_wgs(), tiles);
  if (S > passes) S = passes;
  if (S < 1) S = 1;
  return tg::cdiv(passes, S) * GD_PASS;
}

// out[z][t][j] (z = blockIdx.y; row stride ldo, split stride zs) = sum over the
// chunk's k of X[t, k] B[j, k]
template <int TT>
__global__ __launch_bounds__(256) void lr_down_gemv_kernel(
    const void *__restrict__ X, int x_dt, int T, int64_t ldx, int xvec,
    const void *__restrict__ B, int b_dt, int r, int64_t ldb, int bvec, int n, int chunk,
    float *__restrict__ out, int64_t ldo, int64_t zs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * GD_WAVES + wave;
  const int jc = min(j, r - 1);  // waves past r read the last row and write nothing
  const int k0 = blockIdx.y * chunk, k1 = min(n, k0 + chunk);
  float acc[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) acc[t] = 0.f;
  for (int k = k0 + lane * 8; k < k1; k += GD_PASS) {  // n % 8 == 0: a group of 8 never straddles n
    float b[8];
    load8(B, b_dt, int64_t(jc) * ldb + k, bvec, b);
#pragma unroll
    for (int t = 0; t < TT; ++t) {
      float x[8];
      load8(X, x_dt, int64_t(min(t, T - 1)) * ldx + k, xvec, x);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[t] = fmaf(x[e], b[e], acc[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < TT; ++t) {
    float v = acc[t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0 && t < T && j < r) out[int64_t(blockIdx.y) * zs + int64_t(t) * ldo + j] = v;
  }
}

// ---------------------------------------------------------------------------
// tg_lr_down, mfma regime
// ---------------------------------------------------------------------------
constexpr int MD_BM = 128;            // rows of X per workgroup, 32 per wave
constexpr int MD_BN = 32;             // rows of B per workgroup
constexpr int MD_TK = 32;             // K slab
constexpr int MD_KP = MD_TK / 2 + 4;  // floats per (k parity, row) run, padded (80 B, bank spread)
constexpr int MD_MIN_SLABS = 8;       // a split has at least 256 k

// TG_LR_MIN_SLABS (development switch, read per call; tools/lrc_bench.py sweeps it)
int min_slabs() {
  const char *e = getenv("TG_LR_MIN_SLABS");
  const int v = e ? atoi(e) : 0;
  return v > 0 ? v : MD_MIN_SLABS;
}

int mfma_slabs_per_split(int T, int r, int n) {
  const int nslab = tg::cdiv(n, MD_TK);
  const int64_t tiles = int64_t(tg::cdiv(r, MD_BN)) * tg::cdiv(T, MD_BM);
  int64_t S = (target_wgs() + tiles - 1) / tiles;
  const int s_max = nslab / min_slabs() > 1 ? nslab / min_slabs() : 1;
  if (S > s_max) S = s_max;
  if (S < 1) S = 1;
  return tg::cdiv(nslab, S);
}

// Slabs [blockIdx.z * sps, + sps).  The next slab's X and B are fetched into
// registers before the MFMAs of the current one.  LDS image: [k parity][row]
// [k / 2], so one 16-byte read feeds four k-steps of v_mfma_f32_32x32x2_f32
// (lane l: A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]).
__global__ __launch_bounds__(256) void lr_down_mfma_kernel(
    const void *__restrict__ X, int x_dt, int T, int64_t ldx, int xvec,
    const void *__restrict__ B, int b_dt, int r, int64_t ldb, int bvec, int n, int sps,
    float *__restrict__ out, int64_t ldo, int64_t zs) {
  __shared__ __attribute__((aligned(16))) float Xs[2][MD_BM][MD_KP];
  __shared__ __attribute__((aligned(16))) float Bs[2][MD_BN][MD_KP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, l32 = lane & 31;
  const int row0 = blockIdx.y * MD_BM, col0 = blockIdx.x * MD_BN;
  const int k0 = blockIdx.z * sps * MD_TK, k1 = min(n, k0 + sps * MD_TK);
  floatx16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  // staging: groups of 8 k; X 128 rows x 4 groups = 2 per thread, B 32 x 4 = threads 0 .. 127
  float xr[2][8], br[8];
  auto fetch = [&](int ks) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int v = tid + 256 * i;
      const int gr = row0 + (v >> 2), gk = ks + (v & 3) * 8;
      if (gr < T && gk < k1) {
        load8(X, x_dt, int64_t(gr) * ldx + gk, xvec, xr[i]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) xr[i][e] = 0.f;
      }
    }
    if (tid < 4 * MD_BN) {
      const int gj = col0 + (tid >> 2), gk = ks + (tid & 3) * 8;
      if (gj < r && gk < k1) {
        load8(B, b_dt, int64_t(gj) * ldb + gk, bvec, br);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) br[e] = 0.f;
      }
    }
  };
  fetch(k0);
  for (int ks = k0; ks < k1; ks += MD_TK) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int v = tid + 256 * i, row = v >> 2, g4 = (v & 3) * 4;
      *reinterpret_cast<float4 *>(&Xs[0][row][g4]) =
          make_float4(xr[i][0], xr[i][2], xr[i][4], xr[i][6]);
      *reinterpret_cast<float4 *>(&Xs[1][row][g4]) =
          make_float4(xr[i][1], xr[i][3], xr[i][5], xr[i][7]);
    }
    if (tid < 4 * MD_BN) {
      const int row = tid >> 2, g4 = (tid & 3) * 4;
      *reinterpret_cast<float4 *>(&Bs[0][row][g4]) = make_float4(br[0], br[2], br[4], br[6]);
      *reinterpret_cast<float4 *>(&Bs[1][row][g4]) = make_float4(br[1], br[3], br[5], br[7]);
    }
    __syncthreads();
    if (ks + MD_TK < k1) fetch(ks + MD_TK);
#pragma unroll
    for (int c = 0; c < MD_TK / 8; ++c) {
      const float4 xa = *reinterpret_cast<const float4 *>(&Xs[h][wave * 32 + l32][4 * c]);
      const float4 xb = *reinterpret_cast<const float4 *>(&Bs[h][l32][4 * c]);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa.x, xb.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa.y, xb.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa.z, xb.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa.w, xb.w, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  // C/D: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int col = col0 + l32;
  if (col >= r) return;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = row0 + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
    if (row < T) out[int64_t(blockIdx.z) * zs + int64_t(row) * ldo + col] = acc[e];
  }
}

// TG_LR_DOWN (read per call): 0 auto, 1 gemv (T <= 16), 2 mfma
int lr_down_mode() {
  const char *e = getenv("TG_LR_DOWN");
  if (e && strcmp(e, "gemv") == 0) return 1;
  if (e && strcmp(e, "mfma") == 0) return 2;
  return 0;
}

int gemv_splits(int r, int n) { return tg::cdiv(n, gemv_chunk(r, n)); }
int mfma_splits(int T, int r, int n) {
  return tg::cdiv(tg::cdiv(n, MD_TK), mfma_slabs_per_split(T, r, n));
}

// ---------------------------------------------------------------------------
// tg_lr_finish
// ---------------------------------------------------------------------------
constexpr int FN_FEAT = 64;   // output features per workgroup, one per lane
constexpr int FN_TT = 8;      // rows per wave
constexpr int FN_ROWS = 32;   // rows per workgroup (4 waves)
constexpr int FN_JC = 32;     // directions of A held in registers at a time

// A lane owns one output feature o and FN_TT rows: A[o, :] passes through its
// registers FN_JC directions at a time, Z of the workgroup's rows sits in LDS
// and is read as a broadcast.  Per (t, o) the fma chain runs in ascending j.
__global__ __launch_bounds__(256) void lr_finish_kernel(
    const float *Y32, int64_t ldy32, const float *__restrict__ Z, int64_t ldz,
    const void *__restrict__ A, int a_dt, int64_t lda, int avec, int T, int m, int r,
    const void *__restrict__ bias, int bias_dt, void *Y, int y_dt, int64_t ldy) {
  __shared__ __attribute__((aligned(16))) float zt[FN_ROWS][LR_MAX_RANK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = blockIdx.y * FN_ROWS;
  for (int idx = tid; idx < FN_ROWS * r; idx += 256) {
    const int tt = idx / r, j = idx - tt * r;
    zt[tt][j] = t0 + tt < T ? Z[int64_t(t0 + tt) * ldz + j] : 0.f;
  }
  __syncthreads();
  const int tw = t0 + wave * FN_TT;
  if (tw >= T) return;
  const int o = blockIdx.x * FN_FEAT + lane;
  const int oc = min(o, m - 1);  // lanes past m read the last feature and write nothing
  float v[FN_TT];
#pragma unroll
  for (int t = 0; t < FN_TT; ++t) v[t] = Y32[int64_t(min(tw + t, T - 1)) * ldy32 + oc];
  for (int jc = 0; jc < r; jc += FN_JC) {
    float a[FN_JC];
#pragma unroll
    for (int q = 0; q < FN_JC / 8; ++q) {
      const int j8 = jc + 8 * q;
      if (avec && j8 + 8 <= r) {
        load8(A, a_dt, int64_t(oc) * lda + j8, true, &a[8 * q]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
          a[8 * q + e] = j8 + e < r ? load_as_float(A, a_dt, int64_t(oc) * lda + j8 + e) : 0.f;
      }
    }
    if (jc + FN_JC <= r) {
#pragma unroll
      for (int t = 0; t < FN_TT; ++t)
#pragma unroll
        for (int j = 0; j < FN_JC; ++j) v[t] = fmaf(zt[wave * FN_TT + t][jc + j], a[j], v[t]);
    } else {
#pragma unroll
      for (int t = 0; t < FN_TT; ++t)
#pragma unroll
        for (int j = 0; j < FN_JC; ++j)
          if (jc + j < r) v[t] = fmaf(zt[wave * FN_TT + t][jc + j], a[j], v[t]);
    }
  }
  if (o >= m) return;
  const float bv = bias ? load_as_float(bias, bias_dt, o) : 0.f;
#pragma unroll
  for (int t = 0; t < FN_TT; ++t)
    if (tw + t < T)
      store_from_float(Y, y_dt, int64_t(tw + t) * ldy + o, bias ? v[t] + bv : v[t]);
}

bool dt16(int dt) { return dt == TG_F16 || dt == TG_BF16; }
bool dt_any(int dt) { return dt16(dt) || dt == TG_F32; }

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" size_t tg_lr_down_workspace_size(int T, int r, int n) {
  if (T <= 0 || r <= 0 || n <= 0) return 0;
  // the larger of the two regimes' split counts (TG_LR_DOWN may force either)
  int S = mfma_splits(T, r, n);
  if (T <= GD_MAX_T) S = std::max(S, gemv_splits(r, n));
  if (S <= 1) return 0;  // one split writes Z itself
  return size_t(S) * size_t(T) * size_t(r) * sizeof(float) + 256;
}

extern "C" int tg_lr_down(void *stream, const void *X, int x_dtype, int T, int64_t stride_x,
                          const void *B, int b_dtype, int r, int n, int64_t stride_b, float *Z,
                          int64_t stride_z, void *ws, size_t ws_bytes) {
  TG_ARG(X, 2, "null X");
  TG_ARG(dt16(x_dtype), 3, "x_dtype must be TG_F16 or TG_BF16");
  TG_ARG(T > 0, 4, "T <= 0");
  TG_ARG(B, 6, "null B");
  TG_ARG(dt_any(b_dtype), 7, "b_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(r >= 1 && r <= LR_MAX_RANK, 8, "r must be in [1, 128]");
  TG_ARG(n > 0 && n % 8 == 0, 9, "n must be a positive multiple of 8");
  TG_ARG(stride_x >= n, 5, "stride_x < n");
  TG_ARG(stride_b >= n, 10, "stride_b < n");
  TG_ARG(Z, 11, "null Z");
  TG_ARG(stride_z >= r, 12, "stride_z < r");
  const int mode = lr_down_mode();
  TG_ARG(!(mode == 1 && T > GD_MAX_T), 4, "TG_LR_DOWN=gemv takes T <= 16");
  const bool gemv = mode == 1 || (mode == 0 && T <= GD_AUTO_T);
  TG_ARG(tg::cdiv(T, MD_BM) <= 65535, 4, "T too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int xvec = vec_ok(X, x_dtype, stride_x), bvec = vec_ok(B, b_dtype, stride_b);
  const int S = gemv ? gemv_splits(r, n) : mfma_splits(T, r, n);
  TG_ARG(S <= 65535, 9, "n too large");
  float *out = Z;
  int64_t ldo = stride_z, zs = 0;
  if (S > 1) {
    TG_ARG(ws, 13, "null workspace");
    tg::Arena arena(ws, ws_bytes);
    out = arena.take_aligned<float>(size_t(S) * T * r, 256);
    TG_WS(arena);
    ldo = r;
    zs = int64_t(T) * r;
  }
  if (gemv) {
    const dim3 grid(tg::cdiv(r, GD_WAVES), S);
    const int chunk = gemv_chunk(r, n);
    int TT = 1;
    while (TT < T) TT *= 2;
#define TG_GD(tt)                                                                              \
  hipLaunchKernelGGL(lr_down_gemv_kernel<tt>, grid, dim3(256), 0, st, X, x_dtype, T, stride_x, \
                     xvec, B, b_dtype, r, stride_b, bvec, n, chunk, out, ldo, zs)
    switch (TT) {
      case 1: TG_GD(1); break;
      case 2: TG_GD(2); break;
      case 4: TG_GD(4); break;
      case 8: TG_GD(8); break;
      default: TG_GD(16); break;
    }
#undef TG_GD
  } else {
    const dim3 grid(tg::cdiv(r, MD_BN), tg::cdiv(T, MD_BM), S);
    hipLaunchKernelGGL(lr_down_mfma_kernel, grid, dim3(256), 0, st, X, x_dtype, T, stride_x, xvec,
                       B, b_dtype, r, stride_b, bvec, n, mfma_slabs_per_split(T, r, n), out, ldo,
                       zs);
  }
  TG_LAUNCHED();
  if (S > 1) {
    hipLaunchKernelGGL(qgemv_reduce_kernel, dim3(tg::cdiv(int64_t(T) * r, 256)), dim3(256), 0, st,
                       out, S, T, r, nullptr, TG_F32, Z, TG_F32, stride_z);
    TG_LAUNCHED();
  }
  return 0;
}

extern "C" int tg_lr_finish(void *stream, const float *Y32, int64_t stride_y32, const float *Z,
                            int64_t stride_z, const void *A, int a_dtype, int64_t stride_a, int T,
                            int m, int r, const void *bias, int bias_dtype, void *Y, int y_dtype,
                            int64_t stride_y) {
  TG_ARG(Y32, 2, "null Y32");
  TG_ARG(Z, 4, "null Z");
  TG_ARG(A, 6, "null A");
  TG_ARG(dt_any(a_dtype), 7, "a_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(T > 0, 9, "T <= 0");
  TG_ARG(m > 0, 10, "m <= 0");
  TG_ARG(r >= 1 && r <= LR_MAX_RANK, 11, "r must be in [1, 128]");
  TG_ARG(stride_y32 >= m, 3, "stride_y32 < m");
  TG_ARG(stride_z >= r, 5, "stride_z < r");
  TG_ARG(stride_a >= r, 8, "stride_a < r");
  TG_ARG(!bias || dt_any(bias_dtype), 13, "bias_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(Y, 14, "null Y");
  TG_ARG(dt_any(y_dtype), 15, "y_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(stride_y >= m, 16, "stride_y < m");
  TG_ARG(tg::cdiv(T, FN_ROWS) <= 65535, 9, "T too large");
  const dim3 grid(tg::cdiv(m, FN_FEAT), tg::cdiv(T, FN_ROWS));
  hipLaunchKernelGGL(lr_finish_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), Y32,
                     stride_y32, Z, stride_z, A, a_dtype, stride_a, int(vec_ok(A, a_dtype, stride_a)),
                     T, m, r, bias, bias_dtype, Y, y_dtype, stride_y);
  TG_LAUNCHED();
  return 0;
}
