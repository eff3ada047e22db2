// A18: randomised block-Hadamard rotation Q = diag(s) (I_{n/b} (x) H_b) / sqrt(b).
//
//   tg_hadamard      Y = X Q (or X Q^T) on every row, one pass over HBM
//   tg_hadamard_sym  H <- Q^T H Q in place, FP64, mirrored lower triangle
//
// Numerics (fixed, restated on the host in tests/had_ref.py): the input is
// converted exactly to the compute type (f64 for f64 input, f32 otherwise), the
// signs are applied as sign-bit flips, the stages h = 1, 2, 4, ... b/2 run in that
// order and turn every pair (j, j + h), (j mod 2h) < h, into (u + v, u - v), each
// one rounded operation; then one multiply by c = 1/sqrt(b) and one rounding to
// the output type.  The inverse flips the signs after the scale.  How the stages
// are grouped below moves data, never an operation: the add tree of every output
// is the one of the definition.
//
// tg_hadamard: a lane owns 8 consecutive columns (one 16-byte access of a 16-bit
// type), a wave 512.
//  * h = 1, 2, 4 run in the lane's registers;
//  * h = 8 ... 256 exchange with lane ^ 1 ... lane ^ 32: DPP quad_perm (1, 2),
//    ds_swizzle in bit mode (4, 8, 16; the LDS crossbar, no LDS memory) and
//    v_permlane32_swap (32);
//  * b <= 512: a wave owns one (row, 512 columns) item, four items to a workgroup,
//    so decode (T <= 16) is a handful of workgroups and T = 4096 thousands;
//  * b >= 1024: a workgroup of b / 8 threads owns one block.  After the in-wave
//    stages the block goes to LDS once; a thread then holds the b / 512 values
//    j, j + 512, ... for 8 / (b / 512) consecutive j, runs h = 512 ... b/2 in
//    registers, puts them back, and after a barrier every lane picks up its
//    original 8 columns for a 16-byte store.
// A unit reads all its input before it writes, and units are disjoint, so Y may
// be X.
//
// tg_hadamard_sym: the row pass is tg_hadamard's f64 kernel.  The column pass
// keeps lanes across columns (512 contiguous bytes per wave and row) and 32 rows
// of one column in a thread's registers: stages h = S ... 16 S per launch with
// S = 1, 32, 1024 (one to three launches), signs in the first and the scale in
// the last.  A last kernel copies the lower triangle over the upper one through
// 32 x 32 LDS tiles.  No n x n scratch.
#include <algorithm>
#include <cmath>

#include "../../include/truncgptq.h"
#include "common.h"
#include "qdtype.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int HD_E = 8;            // columns per lane
constexpr int HD_CHUNK = 64 * 8;   // columns per wave
constexpr int HD_WAVES = 4;        // items per workgroup, in-wave regime
constexpr int HD_MIN_B = 32, HD_MAX_B = 4096;

// the value of lane ^ M
template <int M>
__device__ inline uint32_t xor_lane(uint32_t v) {
  if constexpr (M == 1) {
    return uint32_t(__builtin_amdgcn_mov_dpp(int(v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
  } else if constexpr (M == 2) {
    return uint32_t(__builtin_amdgcn_mov_dpp(int(v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
  } else if constexpr (M == 4 || M == 8 || M == 16) {
    return uint32_t(__builtin_amdgcn_ds_swizzle(int(v), 0x1F | (M << 10)));    // and 0x1f, xor M
  } else {
    static_assert(M == 32);
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return (threadIdx.x & 32) ? r[0] : r[1];
  }
}
template <int M>
__device__ inline float xor_lane(float v) {
  return __uint_as_float(xor_lane<M>(__float_as_uint(v)));
}
template <int M>
__device__ inline double xor_lane(double v) {
  const uint64_t u = __double_as_longlong(v);
  const uint32_t lo = xor_lane<M>(uint32_t(u)), hi = xor_lane<M>(uint32_t(u >> 32));
  return __longlong_as_double((uint64_t(hi) << 32) | lo);
}

template <class C>
__device__ inline C flip(C v, bool neg) {
  return neg ? -v : v;
}

// ---- 8 consecutive elements of a row <-> registers ---------------------------
template <class C>
__device__ inline void load_e(const void *p, int dt, int64_t i, bool vec, C *o) {
  if (dt == TG_F64) {
    const double *s = static_cast<const double *>(p) + i;
    if (vec) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double2 a = *reinterpret_cast<const double2 *>(s + 2 * q);
        o[2 * q] = C(a.x), o[2 * q + 1] = C(a.y);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = C(s[e]);
    }
  } else if (dt == TG_F32) {
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
  } else {
    const uint16_t *s = static_cast<const uint16_t *>(p) + i;
    uint16_t h[8];
    if (vec) {
      const u32x4 v = *reinterpret_cast<const u32x4 *>(s);
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = uint16_t(v[e >> 1] >> (16 * (e & 1)));
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) h[e] = s[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
      o[e] = dt == TG_F16 ? from_bits<TG_F16>(h[e]) : from_bits<TG_BF16>(h[e]);
  }
}

template <class C>
__device__ inline void store_e(void *p, int dt, int64_t i, bool vec, const C *v) {
  if (dt == TG_F64) {
    double *d = static_cast<double *>(p) + i;
    if (vec) {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<double2 *>(d + 2 * q) = make_double2(double(v[2 * q]), double(v[2 * q + 1]));
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = double(v[e]);
    }
  } else if (dt == TG_F32) {
    float *d = static_cast<float *>(p) + i;
    if (vec) {
      *reinterpret_cast<float4 *>(d) = make_float4(float(v[0]), float(v[1]), float(v[2]), float(v[3]));
      *reinterpret_cast<float4 *>(d + 4) =
          make_float4(float(v[4]), float(v[5]), float(v[6]), float(v[7]));
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = float(v[e]);
    }
  } else {
    uint16_t *d = static_cast<uint16_t *>(p) + i;
    uint16_t h[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      h[e] = dt == TG_F16 ? to_bits<TG_F16>(float(v[e])) : to_bits<TG_BF16>(float(v[e]));
    if (vec) {
      u32x4 w;
#pragma unroll
      for (int q = 0; q < 4; ++q) w[q] = uint32_t(h[2 * q]) | (uint32_t(h[2 * q + 1]) << 16);
      *reinterpret_cast<u32x4 *>(d) = w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) d[e] = h[e];
    }
  }
}

// the 8 sign bits of columns c0 .. c0 + 7 (c0 % 8 == 0)
__device__ inline uint32_t sign8(const int32_t *sign_bits, int c0) {
  return sign_bits ? (uint32_t(sign_bits[c0 >> 5]) >> (c0 & 31)) & 0xFFu : 0u;
}

template <class C, int M>
__device__ inline void lane_stage(C *v, int lane) {
  const bool up = lane & M;
#pragma unroll
  for (int e = 0; e < HD_E; ++e) {
    const C p = xor_lane<M>(v[e]);
    v[e] = up ? p - v[e] : v[e] + p;   // (u + v, u - v), u the lower column
  }
}

// stages h = 1 ... min(b, 512) / 2 of the 512 columns a wave holds
template <class C>
__device__ inline void wave_stages(C *v, int lane, int b) {
#pragma unroll
  for (int h = 1; h < HD_E; h *= 2)
#pragma unroll
    for (int j = 0; j < HD_E; ++j)
      if ((j & h) == 0) {
        const C u = v[j], w = v[j + h];
        v[j] = u + w, v[j + h] = u - w;
      }
  if (b > 8) lane_stage<C, 1>(v, lane);
  if (b > 16) lane_stage<C, 2>(v, lane);
  if (b > 32) lane_stage<C, 4>(v, lane);
  if (b > 64) lane_stage<C, 8>(v, lane);
  if (b > 128) lane_stage<C, 16>(v, lane);
  if (b > 256) lane_stage<C, 32>(v, lane);
}

template <class C>
__device__ inline void scale_round_store(C *v, C c, uint32_t sg, bool inverse, void *Y, int y_dt,
                                         int64_t at, bool yvec) {
#pragma unroll
  for (int e = 0; e < HD_E; ++e) {
    v[e] = v[e] * c;
    if (inverse) v[e] = flip(v[e], (sg >> e) & 1);
  }
  store_e<C>(Y, y_dt, at, yvec, v);
}

// b <= 512: one wave per (row, 512-column chunk); b divides 512 and n, so a lane
// past n has its whole block past n and exchanges only with such lanes
template <class C>
__global__ __launch_bounds__(64 * HD_WAVES) void had_wave_kernel(
    const void *X, int x_dt, int64_t rows, int n, int64_t ldx, int xvec, int b,
    const int32_t *__restrict__ sign_bits, int inverse, double scale, void *Y, int y_dt,
    int64_t ldy, int yvec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = tg::cdiv(n, HD_CHUNK);
  const int64_t item = int64_t(blockIdx.x) * HD_WAVES + wave;
  if (item >= rows * chunks) return;
  const int64_t row = item / chunks;
  const int c0 = int(item - row * chunks) * HD_CHUNK + lane * HD_E;
  const bool live = c0 < n;
  C v[HD_E];
  uint32_t sg = 0;
  if (live) {
    load_e<C>(X, x_dt, row * ldx + c0, xvec, v);
    sg = sign8(sign_bits, c0);
  } else {
#pragma unroll
    for (int e = 0; e < HD_E; ++e) v[e] = C(0);
  }
  if (!inverse)
#pragma unroll
    for (int e = 0; e < HD_E; ++e) v[e] = flip(v[e], (sg >> e) & 1);
  wave_stages<C>(v, lane, b);
  if (live) scale_round_store<C>(v, C(scale), sg, inverse, Y, y_dt, row * ldy + c0, yvec);
}

// b = 1024, 2048, 4096: a workgroup of b / 8 threads per (row, block)
template <class C, int K>
__global__ __launch_bounds__(512) void had_lds_kernel(
    const void *X, int x_dt, int n, int64_t ldx, int xvec, int b,
    const int32_t *__restrict__ sign_bits, int inverse, double scale, void *Y, int y_dt,
    int64_t ldy, int yvec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char had_smem[];
  C *s = reinterpret_cast<C *>(had_smem);
  const int tid = threadIdx.x, lane = tid & 63;
  const int nblk = n / b;
  const int64_t row = blockIdx.x / nblk;
  const int c0 = int(blockIdx.x - row * nblk) * b + tid * HD_E;
  C v[HD_E];
  load_e<C>(X, x_dt, row * ldx + c0, xvec, v);
  const uint32_t sg = sign8(sign_bits, c0);
  if (!inverse)
#pragma unroll
    for (int e = 0; e < HD_E; ++e) v[e] = flip(v[e], (sg >> e) & 1);
  wave_stages<C>(v, lane, HD_CHUNK);
#pragma unroll
  for (int e = 0; e < HD_E; ++e) s[tid * HD_E + e] = v[e];
  __syncthreads();
  // K = b / 512 chunks; this thread: columns j0 .. j0 + 8 / K of every chunk
  constexpr int q = HD_E / K;
  const int j0 = tid * q;
  C w[HD_E];
#pragma unroll
  for (int e = 0; e < HD_E; ++e) w[e] = s[(e / q) * HD_CHUNK + j0 + (e % q)];
  // w[e]: chunk e / q; stage h = 512 g pairs chunks k and k + g, (k & g) == 0
#pragma unroll
  for (int g = 1; g < K; g *= 2)
#pragma unroll
    for (int e = 0; e < HD_E; ++e) {
      const int k = e / q, e2 = e + g * q;
      if ((k & g) == 0) {
        const C u = w[e], x = w[e2];
        w[e] = u + x, w[e2] = u - x;
      }
    }
#pragma unroll
  for (int e = 0; e < HD_E; ++e) s[(e / q) * HD_CHUNK + j0 + (e % q)] = w[e];
  __syncthreads();
#pragma unroll
  for (int e = 0; e < HD_E; ++e) v[e] = s[tid * HD_E + e];
  scale_round_store<C>(v, C(scale), sg, inverse, Y, y_dt, row * ldy + c0, yvec);
}

// ---- tg_hadamard_sym: column pass and mirror ----------------------------------
constexpr int HS_R = 32;   // rows of one column in a thread's registers

// Stages h = S, 2S, ... (R / 2) S along the row index, R = min(32, b / S).  A
// thread owns column blockIdx.x * 64 + threadIdx.x and group g = blockIdx.y * 4
// + threadIdx.y of n / R: rows base + S k, k < R.
__global__ __launch_bounds__(256) void had_col_kernel(double *H, int n, int64_t ld, int b, int S,
                                                      int R, const int32_t *__restrict__ sign_bits,
                                                      int first, int last, double scale) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  const int g = blockIdx.y * 4 + threadIdx.y;
  if (col >= n || g >= n / R) return;
  // inside a block of b rows: index = lo + S k + S R hi, lo < S, hi < b / (S R)
  const int per_blk = b / R, blk = g / per_blk, gi = g - blk * per_blk;
  const int lo = gi % S, hi = gi / S;
  const int base = blk * b + hi * S * R + lo;
  double v[HS_R];
#pragma unroll
  for (int k = 0; k < HS_R; ++k)
    if (k < R) {
      const int r = base + S * k;
      v[k] = H[int64_t(r) * ld + col];
      if (first && sign_bits && ((uint32_t(sign_bits[r >> 5]) >> (r & 31)) & 1)) v[k] = -v[k];
    }
#pragma unroll
  for (int h = 1; h < HS_R; h *= 2)
    if (h < R) {
#pragma unroll
      for (int k = 0; k < HS_R; ++k)
        if ((k & h) == 0 && k + h < R) {
          const double u = v[k], w = v[k + h];
          v[k] = u + w, v[k + h] = u - w;
        }
    }
#pragma unroll
  for (int k = 0; k < HS_R; ++k)
    if (k < R) H[int64_t(base + S * k) * ld + col] = last ? v[k] * scale : v[k];
}

// upper triangle <- mirror of the lower one, 32 x 32 tiles (n % 32 == 0)
__global__ __launch_bounds__(256) void had_mirror_kernel(double *H, int64_t ld) {
  __shared__ double t[32][33];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
  for (int i = ty; i < 32; i += 8) t[i][tx] = H[int64_t(bi * 32 + i) * ld + bj * 32 + tx];
  __syncthreads();
#pragma unroll
  for (int i = ty; i < 32; i += 8)
    if (bi != bj || tx > i) H[int64_t(bj * 32 + i) * ld + bi * 32 + tx] = t[tx][i];
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// may 16-byte accesses be taken at multiples of 8 elements of a row?
bool vec_ok(const void *p, int dt, int64_t ld) {
  const int bytes = dt == TG_F64 ? 8 : dt == TG_F32 ? 4 : 2;
  return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (ld * bytes) % 16 == 0;
}

template <class C>
int launch_rows(hipStream_t st, const void *X, int x_dt, int64_t rows, int n, int64_t ldx, int b,
                const int32_t *sign_bits, int inverse, void *Y, int y_dt, int64_t ldy) {
  const int xvec = vec_ok(X, x_dt, ldx), yvec = vec_ok(Y, y_dt, ldy);
  const double scale = sizeof(C) == 8 ? 1.0 / std::sqrt(double(b))
                                      : double(float(1.0 / std::sqrt(double(b))));
  if (b <= HD_CHUNK) {
    const int64_t items = rows * tg::cdiv(n, HD_CHUNK);
    const int64_t grid = (items + HD_WAVES - 1) / HD_WAVES;
    if (grid > 0x7fffffffLL) return 1;
    hipLaunchKernelGGL(had_wave_kernel<C>, dim3(unsigned(grid)), dim3(64 * HD_WAVES), 0, st, X,
                       x_dt, rows, n, ldx, xvec, b, sign_bits, inverse, scale, Y, y_dt, ldy, yvec);
  } else {
    const int64_t grid = rows * (n / b);
    if (grid > 0x7fffffffLL) return 1;
#define TG_HD(k)                                                                              \
  hipLaunchKernelGGL((had_lds_kernel<C, k>), dim3(unsigned(grid)), dim3(b / HD_E),            \
                     size_t(b) * sizeof(C), st, X, x_dt, n, ldx, xvec, b, sign_bits, inverse, \
                     scale, Y, y_dt, ldy, yvec)
    switch (b / HD_CHUNK) {
      case 2: TG_HD(2); break;
      case 4: TG_HD(4); break;
      default: TG_HD(8); break;
    }
#undef TG_HD
  }
  return 0;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" int tg_hadamard(void *stream, const void *X, int x_dtype, int64_t rows, int n,
                           int64_t stride_x, int block, const int32_t *sign_bits, int inverse,
                           void *Y, int y_dtype, int64_t stride_y) {
  TG_ARG(X, 2, "null X");
  TG_ARG(x_dtype >= TG_F16 && x_dtype <= TG_F64, 3, "x_dtype must be TG_F16, TG_BF16, TG_F32 or TG_F64");
  TG_ARG(rows > 0, 4, "rows <= 0");
  TG_ARG(n > 0, 5, "n <= 0");
  TG_ARG(stride_x >= n, 6, "stride_x < n");
  TG_ARG(pow2(block) && block >= HD_MIN_B && block <= HD_MAX_B, 7,
         "block must be a power of two in [32, 4096]");
  TG_ARG(n % block == 0, 7, "block must divide n");
  TG_ARG(Y, 10, "null Y");
  TG_ARG(y_dtype >= TG_F16 && y_dtype <= TG_F64, 11, "y_dtype must be TG_F16, TG_BF16, TG_F32 or TG_F64");
  TG_ARG((y_dtype == TG_F64) == (x_dtype == TG_F64), 11,
         "y_dtype is TG_F64 exactly when x_dtype is (the compute type follows the input)");
  TG_ARG(stride_y >= n, 12, "stride_y < n");
  TG_ARG(Y != X || (y_dtype == x_dtype && stride_y == stride_x), 10,
         "in place needs equal dtype and stride");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int too_many =
      x_dtype == TG_F64
          ? launch_rows<double>(st, X, x_dtype, rows, n, stride_x, block, sign_bits, inverse, Y,
                                y_dtype, stride_y)
          : launch_rows<float>(st, X, x_dtype, rows, n, stride_x, block, sign_bits, inverse, Y,
                               y_dtype, stride_y);
  TG_ARG(!too_many, 4, "rows too large");
  TG_LAUNCHED();
  return 0;
}

extern "C" int tg_hadamard_sym(void *stream, double *H, int n, int64_t stride_h, int block,
                               const int32_t *sign_bits) {
  TG_ARG(H, 2, "null H");
  TG_ARG(n > 0, 3, "n <= 0");
  TG_ARG(stride_h >= n, 4, "stride_h < n");
  TG_ARG(pow2(block) && block >= HD_MIN_B && block <= HD_MAX_B, 5,
         "block must be a power of two in [32, 4096]");
  TG_ARG(n % block == 0, 5, "block must divide n");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int too_many = launch_rows<double>(st, H, TG_F64, n, n, stride_h, block, sign_bits, 0, H,
                                           TG_F64, stride_h);
  TG_ARG(!too_many, 3, "n too large");
  TG_LAUNCHED();
  const double scale = 1.0 / std::sqrt(double(block));
  for (int S = 1; S < block; S *= HS_R) {
    const int R = std::min(HS_R, block / S);
    const dim3 grid(tg::cdiv(n, 64), tg::cdiv(n / R, 4));
    TG_ARG(grid.y <= 65535, 3, "n too large");
    hipLaunchKernelGGL(had_col_kernel, grid, dim3(64, 4), 0, st, H, n, stride_h, block, S, R,
                       sign_bits, int(S == 1), int(S * R == block), scale);
    TG_LAUNCHED();
  }
  hipLaunchKernelGGL(had_mirror_kernel, dim3(n / 32, n / 32), dim3(256), 0, st, H, stride_h);
  TG_LAUNCHED();
  return 0;
}
