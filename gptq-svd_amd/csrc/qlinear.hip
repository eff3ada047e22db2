// A14: packed inference -- dequantisation of the AutoGPTQ bit stream written by
// tg_pack_codes / tg_pack_zeros (quant.hip) and the fused dequant GEMM
// Y = X * W^T (+ bias) taken straight from the packed words.
//
// Layout: qweight int32 (n*b/32, m), value i of output feature r at bits
// [i*b, i*b+b) of the little-endian stream of column r; qzeros int32
// (G, m*b/32), the same stream along the output features of one group; scales
// (G, m).  32 values are exactly b words (a "unit"), so with n % 32 == 0 every
// straddling value (3-bit: values 10 and 21 of a unit) stays inside the unit
// and the shifts of a unit are compile-time constants of the template on b.
// Consecutive lanes hold consecutive output features: a word row of qweight
// is read coalesced.
//
// Numerics (fixed, reproducible on the host): w = float(code - zero) *
// float(scale), one fp32 multiply of an exact integer, one round-to-nearest-
// even to the 16-bit operand type; products and sums fp32; bias added in fp32;
// one rounding to the output type.
//
// tg_qgemm, two regimes (switch TG_QGEMM = auto | gemv | mfma, read per call):
//  * gemv (T <= 16; auto picks it up to T = 4): a workgroup = 64 output
//    features x 4 waves; the K range is split over blockIdx.y and, inside the
//    workgroup, over the waves.  X of
//    the workgroup's K chunk is staged once in LDS as fp32 and read as a
//    broadcast; zero and scale are loaded once per group.  The waves' sums are
//    added in wave order through LDS and written to the workspace as
//    partial[s][t][r]; a second kernel adds the partials in ascending s, then
//    the bias, and rounds once.  No atomics, no cross-workgroup hand-off: the
//    result is bit-identical from call to call.
//  * mfma (any T): a workgroup owns a 64- or 128-row x 64-feature tile of Y;
//    per K slab of 128 values (4 units, one per wave and output feature) the
//    weight tile is unpacked into LDS in the operand type next to the X tile,
//    and each wave runs mfma_f32_16x16x32 on its quarter.  While the output
//    tiles alone do not fill the device K is split here too, with the same
//    partial-sum workspace and reduction kernel as the gemv regime.
#include <cstdlib>
#include <cstring>

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "../../include/truncgptq.h"
#include "common.h"
#include "qdtype.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// ---- the bit stream ---------------------------------------------------------
// value i (0..31) of a unit held in w[0..B); i, hence every shift, is a
// compile-time constant after unrolling
template <int B>
__device__ inline int unit_value(const uint32_t (&w)[B], int i) {
  const int bit = i * B, wi = bit >> 5, sh = bit & 31;
  uint32_t v = w[wi] >> sh;
  if (sh + B > 32) v |= w[(wi + 1) % B] << (32 - sh);  // a straddle never leaves the unit
  return int(v & ((1u << B) - 1u));
}

// stored zero of output feature r in one qzeros row (nzw words)
__device__ inline int zero_value(const uint32_t *__restrict__ row, int r, int b) {
  const int64_t bit = int64_t(r) * b;
  const int64_t wi = bit >> 5;
  const int sh = int(bit & 31);
  uint32_t v = row[wi] >> sh;
  if (sh + b > 32) v |= row[wi + 1] << (32 - sh);
  return int(v & ((1u << b) - 1u));
}

__device__ inline float scale_value(const void *sc, int sc_dt, int64_t i) {
  return load_as_float(sc, sc_dt, i);
}

// ---- MXFP4 (A15) --------------------------------------------------------------
// The kernels below take a format parameter: FMT_INT decodes (code - zero) *
// scale; FMT_MX (b = 4, g = 32: every unit is its own group) decodes an E2M1
// code against the unit's E8M0 byte, read from the (units x m) byte image with
// one byte per lane.  The grid is looked up doubled, from an 8-byte table, and
// multiplied by half the scale: 2 grid[i] * 2^(byte - 128) is the
// same real number as grid[i] * 2^(byte - 127) and it is rounded once, so the
// bits are those of the contract's single multiply.
enum { FMT_INT = 0, FMT_MX = 1 };

// 2^(byte - 128) by integer shift into the exponent field; bytes 0 and 1 give
// the subnormals 2^-128 and 2^-127
__device__ inline float mx_half_scale(uint32_t byte) {
  return __uint_as_float(byte >= 2u ? (byte - 1u) << 23 : 0x00200000u << (byte & 1u));
}

// Value q (0..7) of a packed word w of eight 4-bit codes (sign in bit 3 of a
// code).  The table {0, .5, 1, 1.5, 2, 3, 4, 6} doubled is eight bytes; one byte
// permute looks up the four even (or odd) codes of the word at once, selected
// by their low three bits, and each byte converts to fp32 on its own.  The sign
// is bit 4 q + 3 of w, shifted to bit 31 and merged under the magnitude.  With
// q a compile-time constant the selector and the permute are shared by the
// word's values.
__device__ inline float mx_value(uint32_t w, int q, float hs) {
  const uint32_t sel = ((q & 1) ? w >> 4 : w) & 0x07070707u;
  const uint32_t g2 = __builtin_amdgcn_perm(0x0c080604u, 0x03020100u, sel);
  const float p = float((g2 >> (8 * (q >> 1))) & 0xffu) * hs;
  const uint32_t sign = w << (28 - 4 * q);
  return __uint_as_float((__float_as_uint(p) & 0x7fffffffu) | (sign & 0x80000000u));
}

// weight i of a unit: s is the scale (FMT_INT) or half the MX scale (FMT_MX)
template <int B, int FMT>
__device__ inline float unit_weight(const uint32_t (&w)[B], int i, int z, float s) {
  if constexpr (FMT == FMT_MX) return mx_value(w[i >> 3], i & 7, s);  // B == 4: 8 codes a word
  else return float(unit_value<B>(w, i) - z) * s;
}

// ---------------------------------------------------------------------------
// tg_dequant_packed: lane = output feature, blockIdx.y = unit of 32 values.
// General n (the last unit may be short) and any group dividing n.
// ---------------------------------------------------------------------------
template <int B, int FMT = FMT_INT>
__global__ __launch_bounds__(256) void dequant_kernel(const uint32_t *__restrict__ qw,
                                                      const uint32_t *__restrict__ qz,
                                                      const void *__restrict__ sc, int sc_dt,
                                                      int m, int n, int g, void *__restrict__ out,
                                                      int out_dt, int64_t ldo) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= m) return;
  const int u = blockIdx.y;
  const int64_t nw = (int64_t(n) * B) >> 5, nzw = (int64_t(m) * B) >> 5;
  uint32_t w[B];
#pragma unroll
  for (int j = 0; j < B; ++j) {
    const int64_t wi = int64_t(u) * B + j;
    w[j] = wi < nw ? qw[wi * m + r] : 0u;
  }
  int cur = -1, z = 0;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const int k = u * 32 + i;
    if (k < n) {
      const int gi = k / g;
      if (gi != cur) {
        cur = gi;
        if constexpr (FMT == FMT_MX) {
          s = mx_half_scale(static_cast<const uint8_t *>(sc)[int64_t(gi) * m + r]);
        } else {
          z = zero_value(qz + int64_t(gi) * nzw, r, B);
          s = scale_value(sc, sc_dt, int64_t(gi) * m + r);
        }
      }
      store_from_float(out, out_dt, int64_t(r) * ldo + k, unit_weight<B, FMT>(w, i, z, s));
    }
  }
}

// ---------------------------------------------------------------------------
// gemv regime
// ---------------------------------------------------------------------------
constexpr int GV_FEAT = 64;          // output features per workgroup (one per lane)
constexpr int GV_WAVES = 4;          // K sub-slices of a workgroup
constexpr int GV_MAX_UNITS = 16;     // K chunk of a workgroup <= 512 values (X in LDS as fp32)
constexpr int GV_MAX_T = 16;         // rows the gemv regime takes
constexpr int GV_AUTO_T = 4;         // rows up to which TG_QGEMM=auto picks it (measured)
constexpr int GV_TARGET_WGS = 1024;  // ~4 workgroups per CU of a 256-CU device

// units of 32 values per workgroup along K; the number of K splits follows
int gemv_units_per_wg(int m, int n) {
  const int units = n / 32, tiles = tg::cdiv(m, GV_FEAT);
  int S = tg::cdiv(GV_TARGET_WGS, tiles);
  const int s_max = tg::cdiv(units, GV_WAVES), s_min = tg::cdiv(units, GV_MAX_UNITS);
  if (S > s_max) S = s_max;
  if (S < s_min) S = s_min;
  if (S < 1) S = 1;
  return tg::cdiv(units, S);
}

// (waves per SIMD bounded from below: without it the scheduler hoists every
// LDS read of a unit and takes all 256 registers)
template <int B, int DT, int TT, int FMT = FMT_INT>
__global__ __launch_bounds__(256, TT >= 16 ? 2 : 4) void qgemv_kernel(const uint16_t *__restrict__ X, int T,
                                                    int64_t ldx, const uint32_t *__restrict__ qw,
                                                    const uint32_t *__restrict__ qz,
                                                    const void *__restrict__ sc, int sc_dt, int m,
                                                    int n, int g, int ub,
                                                    float *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) float xs[TT][GV_MAX_UNITS * 32];
  __shared__ float red[GV_WAVES][TT][GV_FEAT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int units = n / 32;
  const int u0 = blockIdx.y * ub, u1 = min(units, u0 + ub);
  const int k0 = u0 * 32, len = (u1 - u0) * 32;
  for (int idx = tid; idx < TT * len; idx += 256) {
    const int t = idx / len, k = idx - t * len;
    xs[t][k] = t < T ? from_bits<DT>(X[int64_t(t) * ldx + k0 + k]) : 0.f;
  }
  __syncthreads();

  const int r = blockIdx.x * GV_FEAT + lane;
  const int rc = min(r, m - 1);  // lanes past m read the last feature and write nothing
  const int64_t nzw = (int64_t(m) * B) >> 5;
  float acc[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) acc[t] = 0.f;
  const int uw = tg::cdiv(u1 - u0, GV_WAVES);
  const int ua = u0 + wave * uw, ue = min(u1, ua + uw);
  int cur = -1, z = 0;
  float s = 0.f;
  for (int u = ua; u < ue; ++u) {
    uint32_t w[B];
#pragma unroll
    for (int j = 0; j < B; ++j) w[j] = qw[(int64_t(u) * B + j) * m + rc];
    if constexpr (FMT == FMT_MX) {  // a unit is a group: its byte, one per lane
      s = mx_half_scale(static_cast<const uint8_t *>(sc)[int64_t(u) * m + rc]);
    } else {
      const int gi = (u * 32) / g;  // g % 32 == 0: a unit lies in one group
      if (gi != cur) {
        cur = gi;
        z = zero_value(qz + int64_t(gi) * nzw, rc, B);
        s = scale_value(sc, sc_dt, int64_t(gi) * m + rc);
      }
    }
    const int kl = (u - u0) * 32;
#pragma unroll
    for (int i4 = 0; i4 < 8; ++i4) {
      float wv[4];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        wv[c] = from_bits<DT>(to_bits<DT>(unit_weight<B, FMT>(w, i4 * 4 + c, z, s)));
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const float4 x = *reinterpret_cast<const float4 *>(&xs[t][kl + i4 * 4]);
        acc[t] = fmaf(x.x, wv[0], acc[t]);
        acc[t] = fmaf(x.y, wv[1], acc[t]);
        acc[t] = fmaf(x.z, wv[2], acc[t]);
        acc[t] = fmaf(x.w, wv[3], acc[t]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < TT; ++t) red[wave][t][lane] = acc[t];
  __syncthreads();
  for (int idx = tid; idx < TT * GV_FEAT; idx += 256) {
    const int t = idx >> 6, l = idx & 63;
    const int rr = blockIdx.x * GV_FEAT + l;
    if (t < T && rr < m) {
      float v = red[0][t][l];
#pragma unroll
      for (int wv = 1; wv < GV_WAVES; ++wv) v += red[wv][t][l];
      part[(int64_t(blockIdx.y) * T + t) * m + rr] = v;
    }
  }
}

// (qgemv_reduce_kernel, which finishes the partial sums, is in qdtype.h)

// ---------------------------------------------------------------------------
// mfma regime
// ---------------------------------------------------------------------------
constexpr int MF_TILE = 64;   // output features per workgroup; rows of X: BM = 64 or 128
constexpr int MF_KS = 128;    // K slab: 4 units, one per wave
constexpr int MF_LD = MF_KS + 8;  // LDS row stride in 16-bit elements (272 B, a multiple of 16)

template <int DT>
__device__ inline f32x4 mfma16(const uint16_t *a, const uint16_t *b, f32x4 c) {
  if constexpr (DT == TG_F16) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const f16x8 *>(a),
                                                  *reinterpret_cast<const f16x8 *>(b), c, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8 *>(a),
                                                   *reinterpret_cast<const bf16x8 *>(b), c, 0, 0,
                                                   0);
  }
}

// Slabs [blockIdx.z * sps, +sps) of the K range.  part == nullptr (one split):
// bias and the output rounding happen here; otherwise the fp32 tile goes to
// part[z][T][m] and qgemv_reduce_kernel finishes.  The packed words, zero /
// scale and X of slab k+1 are fetched into registers before the MFMAs of slab
// k, so their latency hides behind the matrix work.
template <int B, int DT, int BM, int FMT = FMT_INT>
__global__ __launch_bounds__(256) void qgemm_mfma_kernel(
    const uint16_t *__restrict__ X, int T, int64_t ldx, int xvec,
    const uint32_t *__restrict__ qw, const uint32_t *__restrict__ qz, const void *__restrict__ sc,
    int sc_dt, int m, int n, int g, int sps, float *__restrict__ part,
    const void *__restrict__ bias, int bias_dt, void *__restrict__ Y, int y_dt, int64_t ldy) {
  constexpr int MI = BM / 32;   // 16-row MFMA tiles per wave (a wave owns BM/2 rows x 32 columns)
  constexpr int XV = BM / 16;   // 8-element groups of the X tile per thread
  __shared__ __attribute__((aligned(16))) uint16_t Xs[BM][MF_LD];
  __shared__ __attribute__((aligned(16))) uint16_t Ws[MF_TILE][MF_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int row0 = blockIdx.y * BM, col0 = blockIdx.x * MF_TILE;
  const int units = n / 32;
  const int64_t nzw = (int64_t(m) * B) >> 5;
  const int r = col0 + lane;  // the feature this thread unpacks (unit `wave` of each slab)
  const int ks0 = blockIdx.z * sps * MF_KS, ks1 = min(n, ks0 + sps * MF_KS);
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
      for (int j = 0; j < B; ++j) w[j] = qw[(int64_t(u) * B + j) * m + r];
      if constexpr (FMT == FMT_MX) {
        s = mx_half_scale(static_cast<const uint8_t *>(sc)[int64_t(u) * m + r]);
      } else {
        const int gi = (u * 32) / g;  // g % 32 == 0: a unit lies in one group
        if (gi != cur) {
          cur = gi;
          z = zero_value(qz + int64_t(gi) * nzw, r, B);
          s = scale_value(sc, sc_dt, int64_t(gi) * m + r);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < B; ++j) w[j] = 0u;
    }
    // X tile: BM rows x 128 k as groups of 8 elements, XV per thread
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      const int v = tid + 256 * i;
      const int gr = row0 + (v >> 4), gk = ks + (v & 15) * 8;
      xr[i] = u32x4{0u, 0u, 0u, 0u};
      if (gr < T && gk < n) {  // n % 8 == 0: a group of 8 never straddles n
        const uint16_t *src = X + int64_t(gr) * ldx + gk;
        if (xvec) {
          xr[i] = *reinterpret_cast<const u32x4 *>(src);
        } else {
          xr[i] = u32x4{uint32_t(src[0]) | (uint32_t(src[1]) << 16),
                        uint32_t(src[2]) | (uint32_t(src[3]) << 16),
                        uint32_t(src[4]) | (uint32_t(src[5]) << 16),
                        uint32_t(src[6]) | (uint32_t(src[7]) << 16)};
        }
      }
    }
  };

  fetch(ks0);
  for (int ks = ks0; ks < ks1; ks += MF_KS) {
    // weight tile: Ws[feature][k] = W^[col0 + feature][ks + k]
    {
      uint32_t pk[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const uint32_t lo = to_bits<DT>(unit_weight<B, FMT>(w, 2 * i, z, s));
        const uint32_t hi = to_bits<DT>(unit_weight<B, FMT>(w, 2 * i + 1, z, s));
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
    if (ks + MF_KS < ks1) fetch(ks + MF_KS);
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
    for (int j = 0; j < 2; ++j) {
      const int col = col0 + wc * 32 + j * 16 + (lane & 15);
      if (col >= m) continue;
      const float bv = (bias && !part) ? load_as_float(bias, bias_dt, col) : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = row0 + wr * (BM / 2) + i * 16 + 4 * (lane >> 4) + e;
        if (row >= T) continue;
        if (part) {
          part[(int64_t(blockIdx.z) * T + row) * m + col] = acc[i][j][e];
        } else {
          const float v = bias ? acc[i][j][e] + bv : acc[i][j][e];
          store_from_float(Y, y_dt, int64_t(row) * ldy + col, v);
        }
      }
    }
}

// K slabs per workgroup of the mfma regime: one split once the output tiles
// alone fill the device, otherwise enough splits for ~MF_TARGET_WGS workgroups
// of at least MF_MIN_SLABS slabs
constexpr int MF_TARGET_WGS = 512;
constexpr int MF_MIN_SLABS = 4;
// rows of X per workgroup: 128 (every unpacked weight feeds twice the MFMAs)
// unless that pads the last row tile by 64 rows or more
int mfma_rows(int T) { return (T > 64 && (T % 128 == 0 || T % 128 > 64)) ? 128 : 64; }
int mfma_slabs_per_split(int T, int m, int n) {
  const int nslab = tg::cdiv(n, MF_KS);
  const int64_t tiles = int64_t(tg::cdiv(m, MF_TILE)) * tg::cdiv(T, mfma_rows(T));
  int64_t S = (MF_TARGET_WGS + tiles - 1) / tiles;
  const int s_max = nslab / MF_MIN_SLABS > 1 ? nslab / MF_MIN_SLABS : 1;
  if (S > s_max) S = s_max;
  if (S < 1) S = 1;
  return tg::cdiv(nslab, S);
}

// ---- host dispatch ----------------------------------------------------------
template <int B, int DT, int FMT>
void launch_gemv(hipStream_t st, int TT, dim3 grid, const uint16_t *X, int T, int64_t ldx,
                 const uint32_t *qw, const uint32_t *qz, const void *sc, int sc_dt, int m, int n,
                 int g, int ub, float *part) {
#define TG_GV(tt)                                                                              \
  hipLaunchKernelGGL((qgemv_kernel<B, DT, tt, FMT>), grid, dim3(256), 0, st, X, T, ldx, qw, qz, sc, \
                     sc_dt, m, n, g, ub, part)
  switch (TT) {
    case 1: TG_GV(1); break;
    case 2: TG_GV(2); break;
    case 4: TG_GV(4); break;
    case 8: TG_GV(8); break;
    default: TG_GV(16); break;
  }
#undef TG_GV
}

template <int B, int FMT = FMT_INT>
void launch_gemv_b(hipStream_t st, int dt, int TT, dim3 grid, const uint16_t *X, int T,
                   int64_t ldx, const uint32_t *qw, const uint32_t *qz, const void *sc, int sc_dt,
                   int m, int n, int g, int ub, float *part) {
  if (dt == TG_F16) launch_gemv<B, TG_F16, FMT>(st, TT, grid, X, T, ldx, qw, qz, sc, sc_dt, m, n, g, ub, part);
  else launch_gemv<B, TG_BF16, FMT>(st, TT, grid, X, T, ldx, qw, qz, sc, sc_dt, m, n, g, ub, part);
}

template <int B, int FMT = FMT_INT>
void launch_mfma_b(hipStream_t st, int dt, dim3 grid, const uint16_t *X, int T, int64_t ldx,
                   int xvec, const uint32_t *qw, const uint32_t *qz, const void *sc, int sc_dt,
                   int m, int n, int g, int sps, float *part, const void *bias, int bias_dt,
                   void *Y, int y_dt, int64_t ldy) {
#define TG_MFK(DT_, BM_)                                                                       \
  hipLaunchKernelGGL((qgemm_mfma_kernel<B, DT_, BM_, FMT>), grid, dim3(256), 0, st, X, T, ldx, xvec, \
                     qw, qz, sc, sc_dt, m, n, g, sps, part, bias, bias_dt, Y, y_dt, ldy)
  const bool big = mfma_rows(T) == 128;
  if (dt == TG_F16) {
    if (big) TG_MFK(TG_F16, 128);
    else TG_MFK(TG_F16, 64);
  } else {
    if (big) TG_MFK(TG_BF16, 128);
    else TG_MFK(TG_BF16, 64);
  }
#undef TG_MFK
}

// TG_QGEMM (read per call): 0 auto (gemv up to T = 4, mfma above), 1 gemv (T <= 16), 2 mfma
int qgemm_mode() {
  const char *e = getenv("TG_QGEMM");
  if (e && strcmp(e, "gemv") == 0) return 1;
  if (e && strcmp(e, "mfma") == 0) return 2;
  return 0;
}

bool bits_ok(int b) { return b == 2 || b == 3 || b == 4 || b == 8; }

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" int tg_dequant_packed(void *stream, const int32_t *qweight, const int32_t *qzeros,
                                 const void *scales, int scale_dtype, int m, int n, int group,
                                 int w_bits, void *out, int out_dtype, int64_t ldo) {
  TG_ARG(qweight, 2, "null qweight");
  TG_ARG(qzeros, 3, "null qzeros");
  TG_ARG(scales, 4, "null scales");
  TG_ARG(scale_dtype == TG_F16 || scale_dtype == TG_F32, 5, "scale_dtype must be TG_F16 or TG_F32");
  TG_ARG(m > 0, 6, "m <= 0");
  TG_ARG(n > 0, 7, "n <= 0");
  TG_ARG(bits_ok(w_bits), 9, "w_bits must be 2, 3, 4 or 8");
  TG_ARG((int64_t(n) * w_bits) % 32 == 0, 7, "n * w_bits must be a multiple of 32");
  TG_ARG((int64_t(m) * w_bits) % 32 == 0, 6, "m * w_bits must be a multiple of 32");
  const int g = group > 0 ? group : n;
  TG_ARG(n % g == 0, 8, "group must divide n");
  TG_ARG(out, 10, "null output");
  TG_ARG(out_dtype == TG_F16 || out_dtype == TG_BF16 || out_dtype == TG_F32, 11,
         "out_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(ldo >= n, 12, "ldo < n");
  const int units = tg::cdiv(n, 32);
  TG_ARG(units <= 65535, 7, "n too large");
  const dim3 grid(tg::cdiv(m, 256), units);
  hipStream_t st = (hipStream_t)stream;
  const uint32_t *qw = reinterpret_cast<const uint32_t *>(qweight);
  const uint32_t *qz = reinterpret_cast<const uint32_t *>(qzeros);
#define TG_DQ(b)                                                                              \
  hipLaunchKernelGGL(dequant_kernel<b>, grid, dim3(256), 0, st, qw, qz, scales, scale_dtype, m, \
                     n, g, out, out_dtype, ldo)
  switch (w_bits) {
    case 2: TG_DQ(2); break;
    case 3: TG_DQ(3); break;
    case 4: TG_DQ(4); break;
    default: TG_DQ(8); break;
  }
#undef TG_DQ
  TG_LAUNCHED();
  return 0;
}

extern "C" size_t tg_qgemm_workspace_size(int T, int m, int n) {
  if (T <= 0 || m <= 0 || n < 32) return 0;
  // the larger of the two regimes' split counts (TG_QGEMM may force either)
  int S = tg::cdiv(tg::cdiv(n, MF_KS), mfma_slabs_per_split(T, m, n));
  if (T <= GV_MAX_T) {
    const int Sg = tg::cdiv(n / 32, gemv_units_per_wg(m, n));
    if (Sg > S) S = Sg;
  }
  if (S <= 1 && T > GV_MAX_T) return 0;  // one split of the mfma regime writes Y directly
  return size_t(S) * size_t(T) * size_t(m) * sizeof(float) + 256;
}

struct QgemmIdx { int T, n, ws; };
static int qgemm_run(const QgemmIdx &ix, int fmt, void *stream, const void *X, int x_dtype, int T,
                     int64_t ldx, const int32_t *qweight, const int32_t *qzeros,
                     const void *scales, int scale_dtype, int m, int n, int g, int w_bits,
                     const void *bias, int bias_dtype, void *Y, int y_dtype, int64_t ldy, void *ws,
                     size_t ws_bytes);

extern "C" int tg_qgemm(void *stream, const void *X, int x_dtype, int T, int64_t ldx,
                        const int32_t *qweight, const int32_t *qzeros, const void *scales,
                        int scale_dtype, int m, int n, int group, int w_bits, const void *bias,
                        int bias_dtype, void *Y, int y_dtype, int64_t ldy, void *ws,
                        size_t ws_bytes) {
  TG_ARG(X, 2, "null X");
  TG_ARG(x_dtype == TG_F16 || x_dtype == TG_BF16, 3, "x_dtype must be TG_F16 or TG_BF16");
  TG_ARG(T > 0, 4, "T <= 0");
  TG_ARG(qweight, 6, "null qweight");
  TG_ARG(qzeros, 7, "null qzeros");
  TG_ARG(scales, 8, "null scales");
  TG_ARG(scale_dtype == TG_F16 || scale_dtype == TG_F32, 9, "scale_dtype must be TG_F16 or TG_F32");
  TG_ARG(m > 0, 10, "m <= 0");
  TG_ARG(n > 0 && n % 32 == 0, 11, "n must be a positive multiple of 32");
  TG_ARG(ldx >= n, 5, "ldx < n");
  TG_ARG(bits_ok(w_bits), 13, "w_bits must be 2, 3, 4 or 8");
  TG_ARG((int64_t(m) * w_bits) % 32 == 0, 10, "m * w_bits must be a multiple of 32");
  const int g = group > 0 ? group : n;
  TG_ARG(g % 32 == 0 && n % g == 0, 12, "group must be a multiple of 32 that divides n");
  TG_ARG(!bias || bias_dtype == TG_F16 || bias_dtype == TG_BF16 || bias_dtype == TG_F32, 15,
         "bias_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(Y, 16, "null Y");
  TG_ARG(y_dtype == x_dtype || y_dtype == TG_F32, 17, "y_dtype must be x_dtype or TG_F32");
  TG_ARG(ldy >= m, 18, "ldy < m");
  return qgemm_run(QgemmIdx{4, 11, 19}, FMT_INT, stream, X, x_dtype, T, ldx, qweight, qzeros, scales,
                   scale_dtype, m, n, g, w_bits, bias, bias_dtype, Y, y_dtype, ldy, ws, ws_bytes);
}

// The dispatch behind tg_qgemm (FMT_INT) and tg_qgemm_mx (FMT_MX: w_bits = 4,
// g = 32, scales = the E8M0 byte image, qzeros unused); arguments checked, ix
// holds the caller's argument indices for the checks that depend on the regime.
static int qgemm_run(const QgemmIdx &ix, int fmt, void *stream, const void *X, int x_dtype, int T,
                     int64_t ldx, const int32_t *qweight, const int32_t *qzeros,
                     const void *scales, int scale_dtype, int m, int n, int g, int w_bits,
                     const void *bias, int bias_dtype, void *Y, int y_dtype, int64_t ldy, void *ws,
                     size_t ws_bytes) {
  const int mode = qgemm_mode();
  TG_ARG(!(mode == 1 && T > GV_MAX_T), ix.T, "TG_QGEMM=gemv takes T <= 16");
  const bool gemv = mode == 1 || (mode == 0 && T <= GV_AUTO_T);
  hipStream_t st = (hipStream_t)stream;
  const uint16_t *Xp = static_cast<const uint16_t *>(X);
  const uint32_t *qw = reinterpret_cast<const uint32_t *>(qweight);
  const uint32_t *qz = reinterpret_cast<const uint32_t *>(qzeros);

  if (gemv) {
    const int ub = gemv_units_per_wg(m, n);
    const int S = tg::cdiv(n / 32, ub);
    TG_ARG(ws, ix.ws, "null workspace");
    tg::Arena arena(ws, ws_bytes);
    float *part = arena.take_aligned<float>(size_t(S) * T * m, 256);
    TG_WS(arena);
    int TT = 1;
    while (TT < T) TT *= 2;
    const dim3 grid(tg::cdiv(m, GV_FEAT), S);
    TG_ARG(S <= 65535, ix.n, "n too large");
    if (fmt == FMT_MX)
      launch_gemv_b<4, FMT_MX>(st, x_dtype, TT, grid, Xp, T, ldx, qw, qz, scales, scale_dtype, m, n, g, ub, part);
    else switch (w_bits) {
      case 2: launch_gemv_b<2>(st, x_dtype, TT, grid, Xp, T, ldx, qw, qz, scales, scale_dtype, m, n, g, ub, part); break;
      case 3: launch_gemv_b<3>(st, x_dtype, TT, grid, Xp, T, ldx, qw, qz, scales, scale_dtype, m, n, g, ub, part); break;
      case 4: launch_gemv_b<4>(st, x_dtype, TT, grid, Xp, T, ldx, qw, qz, scales, scale_dtype, m, n, g, ub, part); break;
      default: launch_gemv_b<8>(st, x_dtype, TT, grid, Xp, T, ldx, qw, qz, scales, scale_dtype, m, n, g, ub, part); break;
    }
    TG_LAUNCHED();
    hipLaunchKernelGGL(qgemv_reduce_kernel, dim3(tg::cdiv(int64_t(T) * m, 256)), dim3(256), 0, st,
                       part, S, T, m, bias, bias_dtype, Y, y_dtype, ldy);
    TG_LAUNCHED();
    return 0;
  }

  TG_ARG(tg::cdiv(T, mfma_rows(T)) <= 65535, ix.T, "T too large");
  const int sps = mfma_slabs_per_split(T, m, n);
  const int S = tg::cdiv(tg::cdiv(n, MF_KS), sps);
  float *part = nullptr;
  if (S > 1) {
    TG_ARG(ws, ix.ws, "null workspace");
    tg::Arena arena(ws, ws_bytes);
    part = arena.take_aligned<float>(size_t(S) * T * m, 256);
    TG_WS(arena);
  }
  const dim3 grid(tg::cdiv(m, MF_TILE), tg::cdiv(T, mfma_rows(T)), S);
  const int xvec = (reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % 8 == 0) ? 1 : 0;
#define TG_MF(b)                                                                               \
  launch_mfma_b<b>(st, x_dtype, grid, Xp, T, ldx, xvec, qw, qz, scales, scale_dtype, m, n, g, sps, \
                   part, bias, bias_dtype, Y, y_dtype, ldy)
  if (fmt == FMT_MX)
    launch_mfma_b<4, FMT_MX>(st, x_dtype, grid, Xp, T, ldx, xvec, qw, qz, scales, scale_dtype, m, n, g,
                             sps, part, bias, bias_dtype, Y, y_dtype, ldy);
  else switch (w_bits) {
    case 2: TG_MF(2); break;
    case 3: TG_MF(3); break;
    case 4: TG_MF(4); break;
    default: TG_MF(8); break;
  }
#undef TG_MF
  TG_LAUNCHED();
  if (S > 1) {
    hipLaunchKernelGGL(qgemv_reduce_kernel, dim3(tg::cdiv(int64_t(T) * m, 256)), dim3(256), 0, st,
                       part, S, T, m, bias, bias_dtype, Y, y_dtype, ldy);
    TG_LAUNCHED();
  }
  return 0;
}

// ---------------------------------------------------------------------------
// A15: MXFP4
// ---------------------------------------------------------------------------
extern "C" int tg_dequant_mx(void *stream, const int32_t *qweight, const uint8_t *scales_e8m0,
                             int fmt, int m, int n, void *out, int out_dtype, int64_t ldo) {
  TG_ARG(qweight, 2, "null qweight");
  TG_ARG(scales_e8m0, 3, "null scales");
  TG_ARG(fmt == TG_FMT_MXFP4, 4, "fmt must be TG_FMT_MXFP4");
  TG_ARG(m > 0, 5, "m <= 0");
  TG_ARG((int64_t(m) * 4) % 32 == 0, 5, "m * 4 must be a multiple of 32");
  TG_ARG(n > 0 && n % 32 == 0, 6, "n must be a positive multiple of 32");
  TG_ARG(out, 7, "null output");
  TG_ARG(out_dtype == TG_F16 || out_dtype == TG_BF16 || out_dtype == TG_F32, 8,
         "out_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(ldo >= n, 9, "ldo < n");
  const int units = n / 32;
  TG_ARG(units <= 65535, 6, "n too large");
  hipLaunchKernelGGL((dequant_kernel<4, FMT_MX>), dim3(tg::cdiv(m, 256), units), dim3(256), 0,
                     (hipStream_t)stream, reinterpret_cast<const uint32_t *>(qweight),
                     (const uint32_t *)nullptr, scales_e8m0, 0, m, n, 32, out, out_dtype, ldo);
  TG_LAUNCHED();
  return 0;
}

extern "C" int tg_qgemm_mx(void *stream, const void *X, int x_dtype, int T, int64_t ldx,
                           const int32_t *qweight, const uint8_t *scales_e8m0, int fmt, int m,
                           int n, const void *bias, int bias_dtype, void *Y, int y_dtype,
                           int64_t ldy, void *ws, size_t ws_bytes) {
  TG_ARG(X, 2, "null X");
  TG_ARG(x_dtype == TG_F16 || x_dtype == TG_BF16, 3, "x_dtype must be TG_F16 or TG_BF16");
  TG_ARG(T > 0, 4, "T <= 0");
  TG_ARG(qweight, 6, "null qweight");
  TG_ARG(scales_e8m0, 7, "null scales");
  TG_ARG(fmt == TG_FMT_MXFP4, 8, "fmt must be TG_FMT_MXFP4");
  TG_ARG(m > 0, 9, "m <= 0");
  TG_ARG(n > 0 && n % 32 == 0, 10, "n must be a positive multiple of 32");
  TG_ARG(ldx >= n, 5, "ldx < n");
  TG_ARG((int64_t(m) * 4) % 32 == 0, 9, "m * 4 must be a multiple of 32");
  TG_ARG(!bias || bias_dtype == TG_F16 || bias_dtype == TG_BF16 || bias_dtype == TG_F32, 12,
         "bias_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(Y, 13, "null Y");
  TG_ARG(y_dtype == x_dtype || y_dtype == TG_F32, 14, "y_dtype must be x_dtype or TG_F32");
  TG_ARG(ldy >= m, 15, "ldy < m");
  return qgemm_run(QgemmIdx{4, 10, 16}, FMT_MX, stream, X, x_dtype, T, ldx, qweight, nullptr,
                   scales_e8m0, 0, m, n, 32, 4, bias, bias_dtype, Y, y_dtype, ldy, ws, ws_bytes);
}
