// A16: MXFP8 activations -- the activation quantiser tg_quant_act_mx and the
// block-scaled GEMM tg_qgemm_mx_act, Y = X^ * W^^T (+ bias) on
// v_mfma_scale_f32_16x16x128_f8f6f4: the e4m3 bytes of X^ and the packed E2M1
// words of an MXFP4 checkpoint go to the matrix pipe as they lie in memory, and
// both E8M0 scale bytes ride in a VGPR.  No weight is decoded on the VALU.
//
// Quantiser (contract in include/truncgptq.h): one thread per (row, block of 32
// columns); a = max |x|, byte = max(exponent_field(a) - 8, 0), t = x *
// 2^(127 - byte), q = e4m3fn(t) rounded to nearest even by hand on the f32 bits
// (the subnormals through v_rndne of t * 2^9), saturating at 448; the sign bit of
// q is the sign bit of x, also where q is zero.
//
// GEMM: the activations are quantised once, by that kernel, into the workspace
// (in the A operand's register order, see quant_act_kernel); fusing it into the GEMM would requantise
// every row once per 64-feature tile (64 times at m = 4096).  One kernel for
// every T: a workgroup of four waves owns BM rows x 64 features, BM = 16 (T <=
// 32; the waves side by side along the features) or 64 (2 x 2 waves of 32
// rows x 32 features).  A K step is one MFMA depth, 128 values = 4 blocks.
// Each lane loads its operands straight from global memory into the MFMA
// registers (no LDS, no barrier): 2 x 16 bytes of X^ (a wave: two contiguous
// KB), 4 packed words of W^ and one scale byte each.  Four steps' operands are
// in registers at once: the loads of step s + 3 are issued before the MFMAs of
// step s.
// K is split over blockIdx.z while the output tiles alone do not fill the
// device (the heuristic of tg_qgemm's mfma regime);
// the partial tiles go to the workspace and qgemv_reduce_kernel adds them in
// ascending split order, so the result is bit-identical from call to call.
#include "../../include/truncgptq.h"
#include "common.h"
#include "qdtype.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int E4M3_EMAX = 8;  // 448 = 1.75 * 2^8

// |t| < 512 -> the e4m3fn byte without its sign: round to nearest even,
// subnormals (multiples of 2^-9 below 2^-6) kept, saturation at 448 (0x7e)
__device__ inline uint32_t e4m3_magnitude(float t) {
  const uint32_t u = __float_as_uint(t) & 0x7fffffffu;
  if (u >= (121u << 23)) {  // |t| >= 2^-6: 23 -> 3 mantissa bits, exponent bias 127 -> 7
    const uint32_t r = ((u + 0x7ffffu + ((u >> 20) & 1u)) >> 20) - (120u << 3);
    return r > 0x7eu ? 0x7eu : r;
  }
  return uint32_t(int(rintf(__uint_as_float(u) * 512.f)));  // 0 .. 8; 8 is 2^-6, byte 0x08
}

// One thread per (row, block).  xvec: 16-byte loads; qvec: 16-byte stores.
// FRAG = false: the ABI's image, xq T x n with row stride ldq and xs T x n/32.
// FRAG = true (the GEMM's workspace): the same bytes in the order the MFMA's A
// operand takes them.  Per tile of 16 rows and K step of 128 columns, 2 KB of
// xq: half h (columns [64 h, 64 h + 64) of the step), then lane l = (row & 15) +
// 16 g, then the 16 bytes of columns 64 h + 16 g + [0, 16); and 64 bytes of xs:
// lane (row & 15) + 16 u holds block u of the step.  A wave then loads an operand
// register set as one contiguous KB, where the row-major image costs 16 rows x
// 64 bytes at stride n.
template <int DT, bool FRAG>
__global__ __launch_bounds__(256) void quant_act_kernel(const uint16_t *__restrict__ X, int T,
                                                        int64_t ldx, int n, int xvec,
                                                        uint8_t *__restrict__ xq, int64_t ldq,
                                                        int qvec, uint8_t *__restrict__ xs) {
  const int units = n / 32;
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= int64_t(T) * units) return;
  const int row = int(idx / units), u = int(idx - int64_t(row) * units);
  const uint16_t *src = X + int64_t(row) * ldx + u * 32;
  uint32_t h[16];  // 32 elements, two a word
  if (xvec) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u32x4 v = reinterpret_cast<const u32x4 *>(src)[i];
      h[4 * i] = v[0], h[4 * i + 1] = v[1], h[4 * i + 2] = v[2], h[4 * i + 3] = v[3];
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) h[i] = uint32_t(src[2 * i]) | (uint32_t(src[2 * i + 1]) << 16);
  }
  float x[32];
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    x[i] = from_bits<DT>(uint16_t(h[i >> 1] >> (16 * (i & 1))));
    a = fmaxf(a, fabsf(x[i]));
  }
  const int ef = int(__float_as_uint(a) >> 23);
  const int byte = ef > E4M3_EMAX ? ef - E4M3_EMAX : 0;
  const float up = __uint_as_float(uint32_t(254 - byte) << 23);  // 2^(127 - byte), a normal f32
  uint32_t q[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = 0u;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    const uint32_t b = e4m3_magnitude(x[i] * up) | ((__float_as_uint(x[i]) >> 24) & 0x80u);
    q[i >> 2] |= b << (8 * (i & 3));
  }
  if constexpr (FRAG) {
    const int steps = tg::cdiv(n, 128);
    const int64_t ts = int64_t(row >> 4) * steps + (u >> 2);  // (tile, step)
    const int lr = row & 15, ub = u & 3;
    u32x4 *dst = reinterpret_cast<u32x4 *>(xq + ts * 2048 + (ub >> 1) * 1024);
    dst[lr + 16 * (2 * (ub & 1))] = u32x4{q[0], q[1], q[2], q[3]};
    dst[lr + 16 * (2 * (ub & 1) + 1)] = u32x4{q[4], q[5], q[6], q[7]};
    xs[ts * 64 + lr + 16 * ub] = uint8_t(byte);
    return;
  }
  uint8_t *dst = xq + int64_t(row) * ldq + u * 32;
  if (qvec) {
    reinterpret_cast<u32x4 *>(dst)[0] = u32x4{q[0], q[1], q[2], q[3]};
    reinterpret_cast<u32x4 *>(dst)[1] = u32x4{q[4], q[5], q[6], q[7]};
  } else {
#pragma unroll
    for (int i = 0; i < 32; ++i) dst[i] = uint8_t(q[i >> 2] >> (8 * (i & 3)));
  }
  xs[idx] = uint8_t(byte);
}

template <bool FRAG>
int launch_quant(hipStream_t st, const void *X, int x_dtype, int T, int64_t ldx, int n,
                 uint8_t *xq, int64_t ldq, uint8_t *xs) {
  const int xvec = (reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % 8 == 0) ? 1 : 0;
  const int qvec = (reinterpret_cast<uintptr_t>(xq) % 16 == 0 && ldq % 16 == 0) ? 1 : 0;
  const dim3 grid(tg::cdiv(int64_t(T) * (n / 32), 256));
  const uint16_t *Xp = static_cast<const uint16_t *>(X);
  if (x_dtype == TG_F16)
    hipLaunchKernelGGL((quant_act_kernel<TG_F16, FRAG>), grid, dim3(256), 0, st, Xp, T, ldx, n, xvec, xq,
                       ldq, qvec, xs);
  else
    hipLaunchKernelGGL((quant_act_kernel<TG_BF16, FRAG>), grid, dim3(256), 0, st, Xp, T, ldx, n, xvec, xq,
                       ldq, qvec, xs);
  return 0;
}

// ---------------------------------------------------------------------------
// the block-scaled GEMM
// ---------------------------------------------------------------------------
constexpr int MA_TILE = 64;   // output features per workgroup
constexpr int MA_KS = 128;    // K step: one MFMA depth, 4 blocks of 32
constexpr int MA_TARGET_WGS = 512;
constexpr int MA_MIN_STEPS = 4;
constexpr int MA_SMALL_T = 32;  // rows up to which the 16-row tile is used

// operands of one K step of a wave: MI row tiles of X^, NJ feature tiles of W^
template <int MI, int NJ>
struct Frag {
  u32x4 a[MI][2];   // e4m3 bytes: k = 16 g + [0, 16) and 64 + 16 g + [0, 16), g = lane >> 4
  u32x4 b[NJ];      // packed E2M1 words: k = 32 g + [0, 32)
  uint32_t sa[MI], sb[NJ];
};

// Steps [blockIdx.z * sps, + sps) of the K range.  part == nullptr (one split):
// bias and the output rounding happen here; otherwise the fp32 tile goes to
// part[z][T][m] and qgemv_reduce_kernel finishes.
template <int MI, int NJ, int WR, int WC, int NS>
__global__ __launch_bounds__(256) void qmxact_kernel(
    const uint8_t *__restrict__ xq, const uint8_t *__restrict__ xs, int T,
    const uint32_t *__restrict__ qw, const uint8_t *__restrict__ sc, int m, int n, int sps,
    float *__restrict__ part, const void *__restrict__ bias, int bias_dt, void *__restrict__ Y,
    int y_dt, int64_t ldy) {
  static_assert(WR * WC == 4 && NJ * WC * 16 == MA_TILE);
  constexpr int BM = 16 * MI * WR;
  constexpr bool PARITY = MI * NJ == 1;  // one tile a wave: even and odd steps accumulate apart
  static_assert(NS >= 2 && (!PARITY || NS % 2 == 0));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave / WC, wc = wave % WC;
  const int lr = lane & 15, g = lane >> 4;
  const int row0 = blockIdx.y * BM + wr * MI * 16, col0 = blockIdx.x * MA_TILE + wc * NJ * 16;
  const int units = n / 32;
  const int steps = tg::cdiv(n, MA_KS);
  const int s0 = blockIdx.z * sps, s1 = min(steps, s0 + sps);

  f32x4 acc[MI][NJ], acc2[PARITY ? 1 : MI][PARITY ? 1 : NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (PARITY) acc2[0][0] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Blocks past n (a K tail of one to three blocks inside a step), rows past T
  // and features past m load nothing: their operands are zero, so they add
  // exactly 0 whatever the scale byte (127 there).
  auto fetch = [&](int s, Frag<MI, NJ> &f) {
    const int u = s * 4 + g;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = row0 + i * 16 + lr;
      // the quantiser's FRAG image: (tile, step) -> 2 x 64 lanes x 16 bytes, 64 scale bytes
      const int64_t ts = int64_t(row >> 4) * steps + s;
      const u32x4 *src = reinterpret_cast<const u32x4 *>(xq + ts * 2048) + lane;
      const bool rv = s < s1 && row < T;
      // n % 32 == 0: a run of 16 bytes never straddles n
      f.a[i][0] = (rv && s * MA_KS + 16 * g < n) ? src[0] : u32x4{0u, 0u, 0u, 0u};
      f.a[i][1] = (rv && s * MA_KS + 64 + 16 * g < n) ? src[64] : u32x4{0u, 0u, 0u, 0u};
      f.sa[i] = (rv && u < units) ? uint32_t(xs[ts * 64 + lane]) : 127u;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int o = col0 + j * 16 + lr;
      const bool wv = s < s1 && o < m && u < units;
      f.b[j] = u32x4{0u, 0u, 0u, 0u};
      f.sb[j] = 127u;
      if (wv) {
#pragma unroll
        for (int w = 0; w < 4; ++w) f.b[j][w] = qw[(int64_t(u) * 4 + w) * m + o];
        f.sb[j] = sc[int64_t(u) * m + o];
      }
    }
  };

  // v_mfma_scale_f32_16x16x128_f8f6f4, cbsz = 0 (A e4m3), blgp = 4 (B fp4), as
  // found on the device with one-hot operands (DESIGN.md "MXFP8 activations").
  // With k numbered so that B is contiguous:
  //   B, 4 VGPRs: lane l holds column l & 15, k = 32 (l >> 4) + q in nibble q of
  //     its 128 bits, the low nibble of a byte first: a lane's four qweight
  //     words of one block, in order;
  //   A, 8 VGPRs: lane l holds row l & 15; bytes 0 .. 15 are k = 16 (l >> 4) + j,
  //     bytes 16 .. 31 are k = 64 + 16 (l >> 4) + (j - 16);
  //   scale B: block u of column c is byte opsel of lane c + 16 u's scale VGPR,
  //     the lane that holds the block;
  //   scale A: block u of row r is byte opsel of lane r + 16 u's scale VGPR,
  //     though that lane holds halves of blocks (l >> 4) / 2 and 2 + (l >> 4) / 2;
  //   C/D: col = l & 15, row = 4 (l >> 4) + reg.
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

  // A ring of NS steps' operands in registers, indexed at compile time: the
  // loads of step s + NS - 1 are issued before the MFMAs of step s.  The kernel
  // has no other way to hide the load latency (one to four waves per SIMD).
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

#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = col0 + j * 16 + lr;
      if (col >= m) continue;
      const float bv = (bias && !part) ? load_as_float(bias, bias_dt, col) : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = row0 + i * 16 + 4 * g + e;
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

// rows of X per workgroup: 16 up to T = 32, 64 above.  (A 128-row tile, 4 x 2
// accumulators a wave, measured 3-7% slower at T = 512: it leaves one wave per
// SIMD at m = n = 4096, and every wave fetches its own operands either way.)
int act_rows(int T) { return T <= MA_SMALL_T ? 16 : 64; }

// K steps per workgroup: one split once the output tiles alone fill the device,
// otherwise enough splits for ~MA_TARGET_WGS workgroups of at least
// MA_MIN_STEPS steps (mfma_slabs_per_split of qlinear.hip on this kernel's tiles)
int act_steps_per_split(int T, int m, int n) {
  const int nstep = tg::cdiv(n, MA_KS);
  const int64_t tiles = int64_t(tg::cdiv(m, MA_TILE)) * tg::cdiv(T, act_rows(T));
  int64_t S = (MA_TARGET_WGS + tiles - 1) / tiles;
  const int s_max = nstep / MA_MIN_STEPS > 1 ? nstep / MA_MIN_STEPS : 1;
  if (S > s_max) S = s_max;
  if (S < 1) S = 1;
  return tg::cdiv(nstep, S);
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" int tg_quant_act_mx(void *stream, const void *X, int x_dtype, int T, int64_t stride_x,
                               int n, int act_fmt, uint8_t *xq, int64_t stride_q, uint8_t *xs) {
  TG_ARG(X, 2, "null X");
  TG_ARG(x_dtype == TG_F16 || x_dtype == TG_BF16, 3, "x_dtype must be TG_F16 or TG_BF16");
  TG_ARG(T > 0, 4, "T <= 0");
  TG_ARG(n > 0 && n % 32 == 0, 6, "n must be a positive multiple of 32");
  TG_ARG(stride_x >= n, 5, "stride_x < n");
  TG_ARG(act_fmt == TG_ACT_MXFP8, 7, "act_fmt must be TG_ACT_MXFP8");
  TG_ARG(xq, 8, "null xq");
  TG_ARG(stride_q >= n, 9, "stride_q < n");
  TG_ARG(xs, 10, "null xs");
  launch_quant<false>((hipStream_t)stream, X, x_dtype, T, stride_x, n, xq, stride_q, xs);
  TG_LAUNCHED();
  return 0;
}

extern "C" size_t tg_qgemm_mx_act_workspace_size(int T, int m, int n) {
  if (T <= 0 || m <= 0 || n < 32) return 0;
  tg::Sizer sz;
  const size_t ts = size_t(tg::cdiv(T, 16)) * tg::cdiv(n, MA_KS);  // (tile, step) pairs of X^
  sz.take_aligned<uint8_t>(ts * 2048, 256);
  sz.take_aligned<uint8_t>(ts * 64, 256);
  const int S = tg::cdiv(tg::cdiv(n, MA_KS), act_steps_per_split(T, m, n));
  if (S > 1) sz.take_aligned<float>(size_t(S) * T * m, 256);
  return sz.off;
}

extern "C" int tg_qgemm_mx_act(void *stream, const void *X, int x_dtype, int T, int64_t stride_x,
                               const int32_t *qweight, const uint8_t *scales_e8m0, int fmt,
                               int act_fmt, int m, int n, const void *bias, int bias_dtype,
                               void *Y, int y_dtype, int64_t stride_y, void *ws,
                               size_t ws_bytes) {
  TG_ARG(X, 2, "null X");
  TG_ARG(x_dtype == TG_F16 || x_dtype == TG_BF16, 3, "x_dtype must be TG_F16 or TG_BF16");
  TG_ARG(T > 0, 4, "T <= 0");
  TG_ARG(qweight, 6, "null qweight");
  TG_ARG(scales_e8m0, 7, "null scales");
  TG_ARG(fmt == TG_FMT_MXFP4, 8, "fmt must be TG_FMT_MXFP4");
  TG_ARG(act_fmt == TG_ACT_MXFP8, 9, "act_fmt must be TG_ACT_MXFP8");
  TG_ARG(m > 0, 10, "m <= 0");
  TG_ARG((int64_t(m) * 4) % 32 == 0, 10, "m * 4 must be a multiple of 32");
  TG_ARG(n > 0 && n % 32 == 0, 11, "n must be a positive multiple of 32");
  TG_ARG(stride_x >= n, 5, "stride_x < n");
  TG_ARG(!bias || bias_dtype == TG_F16 || bias_dtype == TG_BF16 || bias_dtype == TG_F32, 13,
         "bias_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(Y, 14, "null Y");
  TG_ARG(y_dtype == TG_F16 || y_dtype == TG_BF16 || y_dtype == TG_F32, 15,
         "y_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(stride_y >= m, 16, "stride_y < m");
  const int BM = act_rows(T);
  TG_ARG(tg::cdiv(T, BM) <= 65535, 4, "T too large");
  TG_ARG(ws, 17, "null workspace");
  const int sps = act_steps_per_split(T, m, n);
  const int S = tg::cdiv(tg::cdiv(n, MA_KS), sps);
  tg::Arena arena(ws, ws_bytes);
  const size_t ts = size_t(tg::cdiv(T, 16)) * tg::cdiv(n, MA_KS);
  uint8_t *xq = arena.take_aligned<uint8_t>(ts * 2048, 256);
  uint8_t *xs = arena.take_aligned<uint8_t>(ts * 64, 256);
  float *part = S > 1 ? arena.take_aligned<float>(size_t(S) * T * m, 256) : nullptr;
  TG_WS(arena);
  hipStream_t st = (hipStream_t)stream;
  launch_quant<true>(st, X, x_dtype, T, stride_x, n, xq, n, xs);
  TG_LAUNCHED();
  const dim3 grid(tg::cdiv(m, MA_TILE), tg::cdiv(T, BM), S);
  const uint32_t *qw = reinterpret_cast<const uint32_t *>(qweight);
#define TG_MA(MI_, NJ_, WR_, WC_, NS_)                                                         \
  hipLaunchKernelGGL((qmxact_kernel<MI_, NJ_, WR_, WC_, NS_>), grid, dim3(256), 0, st, xq, xs, T, \
                     qw, scales_e8m0, m, n, sps, part, bias, bias_dtype, Y, y_dtype, stride_y)
  // four steps in flight (two measured 5-8% slower at T = 512)
  if (BM == 16) TG_MA(1, 1, 1, 4, 4);
  else TG_MA(2, 2, 2, 2, 4);
#undef TG_MA
  TG_LAUNCHED();
  if (S > 1) {
    hipLaunchKernelGGL(qgemv_reduce_kernel, dim3(tg::cdiv(int64_t(T) * m, 256)), dim3(256), 0, st,
                       part, S, T, m, bias, bias_dtype, Y, y_dtype, stride_y);
    TG_LAUNCHED();
  }
  return 0;
}
