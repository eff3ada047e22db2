// A21: packed inference for act-order checkpoints (desc_act = true): the groups
// of the AutoGPTQ layout are taken along a permutation of the input columns,
// g_idx[c] = group of column c, every group with exactly g columns.
//
// The kernels of qlinear.hip fetch one zero and one scale per unit of 32 stream
// positions ("a unit lies in one group"); with act-order the 32 columns of a
// unit belong to up to 32 groups.  Instead of a lookup per column the stream is
// sorted by group once at load and the activation columns are permuted:
//   col_perm = argsort(g_idx, stable)   (host; the columns of group 0 ascending,
//                                        then group 1, ...)
//   sorted stream: position j holds the code of column col_perm[j]
//                                       (tg_repack_gidx, once)
// Position j of the sorted stream lies in group j / g, so zeros and scales are
// the checkpoint's, read exactly as the static kernels read them, and
//   y[t, r] = sum_j x[t, col_perm[j]] * w_sorted[r, j].
//
// tg_qgemm_gidx follows tg_qgemm's choice of regime, so that it computes bit
// for bit what tg_qgemm computes on the sorted stream and x[:, col_perm]:
//  * gemv regime: the gather is fused into the staging of the workgroup's K
//    chunk, xs[t][k] = x[t, col_perm[k0 + k]] (at most 512 two-byte reads per
//    row and workgroup, the rows of x being L2 resident); past the staging it
//    is gemv_accumulate of qgemv.h, the body qgemv_kernel runs, and the same
//    split-K reduce.  No extra launch, no sorted copy of x.
//  * mfma regime: gathering inside the tile kernel would repeat the scattered
//    reads once per 64-feature column tile (m / 64 times); one tg_gather_cols
//    into the workspace amortises them, and tg_qgemm runs on the sorted copy.
//
// col_perm is device memory the host cannot check per call: every kernel reads
// an entry outside [0, n) as column 0, so a bad map gives wrong numbers and
// never an access outside the buffers.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "../../include/truncgptq.h"
#include "common.h"
#include "qdtype.h"
#include "qgemv.h"
#include "qunpack.h"

namespace {

__device__ inline int col_of(const int32_t *__restrict__ cp, int j, int n) {
  const int c = cp[j];
  return unsigned(c) < unsigned(n) ? c : 0;
}

// ---------------------------------------------------------------------------
// tg_repack_gidx: lane = output feature, blockIdx.y = unit of 32 sorted
// positions (B words).  The 32 source columns are uniform over the workgroup;
// every word row is read and written coalesced along m.  A source code may
// straddle two words (3 bits); an output straddle never leaves the unit.
// ---------------------------------------------------------------------------
template <int B>
__global__ __launch_bounds__(256) void repack_kernel(const uint32_t *__restrict__ qw,
                                                     const int32_t *__restrict__ cp, int m, int n,
                                                     uint32_t *__restrict__ out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  const int u = blockIdx.y;
  constexpr uint32_t mask = (1u << B) - 1u;
  uint32_t w[B];
#pragma unroll
  for (int j = 0; j < B; ++j) w[j] = 0u;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const int64_t bit = int64_t(col_of(cp, u * 32 + i, n)) * B;
    const int64_t wi = bit >> 5;
    const int sh = int(bit & 31);
    uint32_t v = qw[wi * m + r] >> sh;
    if (sh + B > 32) v |= qw[(wi + 1) * m + r] << (32 - sh);  // n * B % 32 == 0: wi + 1 exists
    v &= mask;
    const int ob = i * B, ow = ob >> 5, os = ob & 31;  // compile-time after unrolling
    w[ow] |= v << os;
    if (os + B > 32) w[(ow + 1) % B] |= v >> (32 - os);
  }
#pragma unroll
  for (int j = 0; j < B; ++j) out[(int64_t(u) * B + j) * m + r] = w[j];
}

// ---------------------------------------------------------------------------
// tg_gather_cols: Y[t, j] = X[t, col_perm[j]].  A workgroup loads GC_ROWS rows
// of one segment of GC_SEG source columns coalesced into LDS (a whole row up to
// n = GC_SEG), then walks the sorted positions and writes, two per thread and
// coalesced, those whose source lies in its segment: the random access happens
// in LDS only, and col_perm is read once for the GC_ROWS rows.
// ---------------------------------------------------------------------------
constexpr int GC_SEG = 4096;
constexpr int GC_ROWS = 4;

__global__ __launch_bounds__(256) void gather_cols_kernel(const uint16_t *__restrict__ X, int T,
                                                          int64_t ldx, int n, int xvec,
                                                          const int32_t *__restrict__ cp,
                                                          uint16_t *__restrict__ Y, int64_t ldy,
                                                          int yvec) {
  __shared__ __attribute__((aligned(16))) uint16_t seg[GC_ROWS][GC_SEG];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * GC_SEG, cl = min(GC_SEG, n - c0);  // n % 32 == 0, so is cl
  const int t0 = blockIdx.y * GC_ROWS, tr = min(GC_ROWS, T - t0);
  const int gpr = cl >> 3;  // 8-element groups per row
  for (int v = tid; v < tr * gpr; v += 256) {
    const int t = v / gpr, k = (v - t * gpr) * 8;
    const uint16_t *src = X + int64_t(t0 + t) * ldx + c0 + k;
    u32x4 q;
    if (xvec) {
      q = *reinterpret_cast<const u32x4 *>(src);
    } else {
      q = u32x4{uint32_t(src[0]) | (uint32_t(src[1]) << 16),
                uint32_t(src[2]) | (uint32_t(src[3]) << 16),
                uint32_t(src[4]) | (uint32_t(src[5]) << 16),
                uint32_t(src[6]) | (uint32_t(src[7]) << 16)};
    }
    *reinterpret_cast<u32x4 *>(&seg[t][k]) = q;
  }
  __syncthreads();
  for (int p = tid; p < (n >> 1); p += 256) {
    const int a = col_of(cp, 2 * p, n) - c0, b = col_of(cp, 2 * p + 1, n) - c0;
    const bool ina = unsigned(a) < unsigned(cl), inb = unsigned(b) < unsigned(cl);
    if (!ina && !inb) continue;
    for (int t = 0; t < tr; ++t) {
      uint16_t *dst = Y + int64_t(t0 + t) * ldy + 2 * p;
      if (yvec && ina && inb) {
        *reinterpret_cast<uint32_t *>(dst) = uint32_t(seg[t][a]) | (uint32_t(seg[t][b]) << 16);
      } else {
        if (ina) dst[0] = seg[t][a];
        if (inb) dst[1] = seg[t][b];
      }
    }
  }
}

int launch_gather(hipStream_t st, const void *X, int T, int64_t ldx, int n, const int32_t *cp,
                  void *Y, int64_t ldy) {
  const int xvec = (reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % 8 == 0) ? 1 : 0;
  const int yvec = (reinterpret_cast<uintptr_t>(Y) % 4 == 0 && ldy % 2 == 0) ? 1 : 0;
  hipLaunchKernelGGL(gather_cols_kernel, dim3(tg::cdiv(n, GC_SEG), tg::cdiv(T, GC_ROWS)), dim3(256),
                     0, st, static_cast<const uint16_t *>(X), T, ldx, n, xvec, cp,
                     static_cast<uint16_t *>(Y), ldy, yvec);
  return int(hipGetLastError());
}

// ---------------------------------------------------------------------------
// the gemv regime with the gather fused into the staging (geometry, launch
// bounds and everything past the barrier are qgemv_kernel's)
// ---------------------------------------------------------------------------
template <int B, int DT, int TT>
__global__ __launch_bounds__(256, TT >= 16 ? 2 : 4) void qgemv_gidx_kernel(
    const uint16_t *__restrict__ X, int T, int64_t ldx, const int32_t *__restrict__ cp,
    const uint32_t *__restrict__ qw, const uint32_t *__restrict__ qz, const void *__restrict__ sc,
    int sc_dt, int m, int n, int g, int ub, float *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) float xs[TT][GV_MAX_UNITS * 32];
  __shared__ float red[GV_WAVES][TT][GV_FEAT];
  const int tid = threadIdx.x;
  const int units = n / 32;
  const int u0 = blockIdx.y * ub, u1 = min(units, u0 + ub);
  const int k0 = u0 * 32, len = (u1 - u0) * 32;
  for (int k = tid; k < len; k += 256) {
    const int c = col_of(cp, k0 + k, n);
#pragma unroll
    for (int t = 0; t < TT; ++t) xs[t][k] = t < T ? from_bits<DT>(X[int64_t(t) * ldx + c]) : 0.f;
  }
  __syncthreads();
  gemv_accumulate<B, DT, TT, FMT_INT>(xs, red, T, qw, qz, sc, sc_dt, m, g, u0, u1, part);
}

template <int B, int DT>
void launch_gemv_gidx(hipStream_t st, int TT, dim3 grid, const uint16_t *X, int T, int64_t ldx,
                      const int32_t *cp, const uint32_t *qw, const uint32_t *qz, const void *sc,
                      int sc_dt, int m, int n, int g, int ub, float *part) {
#define TG_GVX(tt)                                                                                \
  hipLaunchKernelGGL((qgemv_gidx_kernel<B, DT, tt>), grid, dim3(256), 0, st, X, T, ldx, cp, qw, qz, \
                     sc, sc_dt, m, n, g, ub, part)
  switch (TT) {
    case 1: TG_GVX(1); break;
    case 2: TG_GVX(2); break;
    case 4: TG_GVX(4); break;
    case 8: TG_GVX(8); break;
    default: TG_GVX(16); break;
  }
#undef TG_GVX
}

// ---------------------------------------------------------------------------
// tg_dequant_gidx: dequant_kernel of qlinear.hip on the sorted stream, position
// k of unit u stored at column col_perm[k] (n % 32 == 0: no short unit)
// ---------------------------------------------------------------------------
template <int B>
__global__ __launch_bounds__(256) void dequant_gidx_kernel(
    const uint32_t *__restrict__ qw, const uint32_t *__restrict__ qz, const void *__restrict__ sc,
    int sc_dt, const int32_t *__restrict__ cp, int m, int n, int g, void *__restrict__ out,
    int out_dt, int64_t ldo) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  const int u = blockIdx.y;
  const int64_t nzw = (int64_t(m) * B) >> 5;
  uint32_t w[B];
#pragma unroll
  for (int j = 0; j < B; ++j) w[j] = qw[(int64_t(u) * B + j) * m + r];
  int cur = -1, z = 0;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const int k = u * 32 + i;
    const int gi = k / g;
    if (gi != cur) {
      cur = gi;
      z = zero_value(qz + int64_t(gi) * nzw, r, B);
      s = scale_value(sc, sc_dt, int64_t(gi) * m + r);
    }
    store_from_float(out, out_dt, int64_t(r) * ldo + col_of(cp, k, n),
                     unit_weight<B, FMT_INT>(w, i, z, s));
  }
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" int tg_repack_gidx(void *stream, const int32_t *qweight, const int32_t *col_perm, int m,
                              int n, int w_bits, int32_t *out) {
  TG_ARG(qweight, 2, "null qweight");
  TG_ARG(col_perm, 3, "null col_perm");
  TG_ARG(m > 0, 4, "m <= 0");
  TG_ARG(n > 0 && n % 32 == 0, 5, "n must be a positive multiple of 32");
  TG_ARG(n / 32 <= 65535, 5, "n too large");
  TG_ARG(bits_ok(w_bits), 6, "w_bits must be 2, 3, 4 or 8");
  TG_ARG(out, 7, "null output");
  TG_ARG(out != qweight, 7, "out must not alias qweight");
  const dim3 grid(tg::cdiv(m, 256), n / 32);
  with_bits(w_bits, [&](auto b) {
    hipLaunchKernelGGL(repack_kernel<b.value>, grid, dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t *>(qweight), col_perm, m, n,
                       reinterpret_cast<uint32_t *>(out));
  });
  TG_LAUNCHED();
  return 0;
}

extern "C" int tg_gather_cols(void *stream, const void *X, int x_dtype, int T, int64_t stride_x, int n,
                              const int32_t *col_perm, void *Y, int64_t stride_y) {
  TG_ARG(X, 2, "null X");
  TG_ARG(x_dtype == TG_F16 || x_dtype == TG_BF16, 3, "x_dtype must be TG_F16 or TG_BF16");
  TG_ARG(T > 0, 4, "T <= 0");
  TG_ARG(tg::cdiv(T, GC_ROWS) <= 65535, 4, "T too large");
  TG_ARG(n > 0 && n % 32 == 0, 6, "n must be a positive multiple of 32");
  TG_ARG(stride_x >= n, 5, "stride_x < n");
  TG_ARG(col_perm, 7, "null col_perm");
  TG_ARG(Y, 8, "null Y");
  TG_ARG(Y != X, 8, "Y must not alias X");
  TG_ARG(stride_y >= n, 9, "stride_y < n");
  TG_HIP(hipError_t(launch_gather((hipStream_t)stream, X, T, stride_x, n, col_perm, Y, stride_y)));
  return 0;
}

extern "C" size_t tg_qgemm_gidx_workspace_size(int T, int m, int n) {
  if (T <= 0 || m <= 0 || n < 32) return 0;
  // the sorted copy of X (the mfma regime; TG_QGEMM may force it at any T), then tg_qgemm's own
  return size_t(T) * size_t(n) * sizeof(uint16_t) + 256 + tg_qgemm_workspace_size(T, m, n);
}

extern "C" int tg_qgemm_gidx(void *stream, const void *X, int x_dtype, int T, int64_t stride_x,
                             const int32_t *qweight, const int32_t *qzeros, const void *scales,
                             int scale_dtype, int m, int n, int group, int w_bits, const void *bias,
                             int bias_dtype, void *Y, int y_dtype, int64_t stride_y, void *ws,
                             size_t ws_bytes, const int32_t *col_perm) {
  TG_ARG(X, 2, "null X");
  TG_ARG(x_dtype == TG_F16 || x_dtype == TG_BF16, 3, "x_dtype must be TG_F16 or TG_BF16");
  TG_ARG(T > 0, 4, "T <= 0");
  TG_ARG(qweight, 6, "null qweight");
  TG_ARG(qzeros, 7, "null qzeros");
  TG_ARG(scales, 8, "null scales");
  TG_ARG(scale_dtype == TG_F16 || scale_dtype == TG_F32, 9, "scale_dtype must be TG_F16 or TG_F32");
  TG_ARG(m > 0, 10, "m <= 0");
  TG_ARG(n > 0 && n % 32 == 0, 11, "n must be a positive multiple of 32");
  TG_ARG(stride_x >= n, 5, "stride_x < n");
  TG_ARG(bits_ok(w_bits), 13, "w_bits must be 2, 3, 4 or 8");
  TG_ARG((int64_t(m) * w_bits) % 32 == 0, 10, "m * w_bits must be a multiple of 32");
  const int g = group > 0 ? group : n;
  TG_ARG(g % 32 == 0 && n % g == 0, 12, "group must be a multiple of 32 that divides n");
  TG_ARG(!bias || bias_dtype == TG_F16 || bias_dtype == TG_BF16 || bias_dtype == TG_F32, 15,
         "bias_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(Y, 16, "null Y");
  TG_ARG(y_dtype == x_dtype || y_dtype == TG_F32, 17, "y_dtype must be x_dtype or TG_F32");
  TG_ARG(stride_y >= m, 18, "stride_y < m");
  TG_ARG(ws, 19, "null workspace");
  TG_ARG(col_perm, 21, "null col_perm");
  const int mode = qgemm_mode();
  TG_ARG(!(mode == 1 && T > GV_MAX_T), 4, "TG_QGEMM=gemv takes T <= 16");
  hipStream_t st = (hipStream_t)stream;
  tg::Arena arena(ws, ws_bytes);

  if (mode == 1 || (mode == 0 && T <= GV_AUTO_T)) {  // tg_qgemm's rule
    const int ub = gemv_units_per_wg(m, n);
    const int S = tg::cdiv(n / 32, ub);
    TG_ARG(S <= 65535, 11, "n too large");
    float *part = arena.take_aligned<float>(size_t(S) * T * m, 256);
    TG_WS(arena);
    int TT = 1;
    while (TT < T) TT *= 2;
    const dim3 grid(tg::cdiv(m, GV_FEAT), S);
    const uint16_t *Xp = static_cast<const uint16_t *>(X);
    const uint32_t *qw = reinterpret_cast<const uint32_t *>(qweight);
    const uint32_t *qz = reinterpret_cast<const uint32_t *>(qzeros);
    with_bits(w_bits, [&](auto b) {
      if (x_dtype == TG_F16)
        launch_gemv_gidx<b.value, TG_F16>(st, TT, grid, Xp, T, stride_x, col_perm, qw, qz, scales,
                                          scale_dtype, m, n, g, ub, part);
      else
        launch_gemv_gidx<b.value, TG_BF16>(st, TT, grid, Xp, T, stride_x, col_perm, qw, qz, scales,
                                           scale_dtype, m, n, g, ub, part);
    });
    TG_LAUNCHED();
    hipLaunchKernelGGL(qgemv_reduce_kernel, dim3(tg::cdiv(int64_t(T) * m, 256)), dim3(256), 0, st,
                       part, S, T, m, bias, bias_dtype, Y, y_dtype, stride_y);
    TG_LAUNCHED();
    return 0;
  }

  TG_ARG(tg::cdiv(T, GC_ROWS) <= 65535, 4, "T too large");
  uint16_t *xsorted = arena.take_aligned<uint16_t>(size_t(T) * n, 256);
  TG_WS(arena);
  TG_HIP(hipError_t(launch_gather(st, X, T, stride_x, n, col_perm, xsorted, n)));
  // the remaining arguments have tg_qgemm's positions: its errors name them rightly
  return tg_qgemm(stream, xsorted, x_dtype, T, n, qweight, qzeros, scales, scale_dtype, m, n, group,
                  w_bits, bias, bias_dtype, Y, y_dtype, stride_y, arena.base + arena.off,
                  ws_bytes - arena.off);
}

extern "C" int tg_dequant_gidx(void *stream, const int32_t *qweight, const int32_t *qzeros,
                               const void *scales, int scale_dtype, int m, int n, int group,
                               int w_bits, void *out, int out_dtype, int64_t stride_o,
                               const int32_t *col_perm) {
  TG_ARG(qweight, 2, "null qweight");
  TG_ARG(qzeros, 3, "null qzeros");
  TG_ARG(scales, 4, "null scales");
  TG_ARG(scale_dtype == TG_F16 || scale_dtype == TG_F32, 5, "scale_dtype must be TG_F16 or TG_F32");
  TG_ARG(m > 0, 6, "m <= 0");
  TG_ARG(n > 0 && n % 32 == 0, 7, "n must be a positive multiple of 32");
  TG_ARG(n / 32 <= 65535, 7, "n too large");
  TG_ARG(bits_ok(w_bits), 9, "w_bits must be 2, 3, 4 or 8");
  TG_ARG((int64_t(m) * w_bits) % 32 == 0, 6, "m * w_bits must be a multiple of 32");
  const int g = group > 0 ? group : n;
  TG_ARG(n % g == 0, 8, "group must divide n");
  TG_ARG(out, 10, "null output");
  TG_ARG(out_dtype == TG_F16 || out_dtype == TG_BF16 || out_dtype == TG_F32, 11,
         "out_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(stride_o >= n, 12, "stride_o < n");
  TG_ARG(col_perm, 13, "null col_perm");
  const dim3 grid(tg::cdiv(m, 256), n / 32);
  with_bits(w_bits, [&](auto b) {
    hipLaunchKernelGGL(dequant_gidx_kernel<b.value>, grid, dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint32_t *>(qweight),
                       reinterpret_cast<const uint32_t *>(qzeros), scales, scale_dtype, col_perm, m,
                       n, g, out, out_dtype, stride_o);
  });
  TG_LAUNCHED();
  return 0;
}
