// A20: INT8 activations for integer checkpoints -- the per-token quantiser
// tg_quant_act_i8 and the W{2,3,4,8}A8 GEMM tg_qgemm_act on the i8 MFMA
// (v_mfma_i32_16x16x64_i8, and v_mfma_i32_16x16x32_i8 where a group boundary
// falls inside a 64-value step).  Contract in include/truncgptq.h.
//
// The zero point is not in the inner loop: sum q (c - z) = sum q c - z sum q, so
// the unsigned codes go to the matrix pipe as they are (8-bit: one xor per word
// recentres them) and z meets the quantiser's per-group sums of q, xsum, once
// per group: D = acc - z' xsum, all in int32, then accf += float(D) * scale.
//
// Integer accumulation is exact, so any assignment of a step's 64 k's to (lane
// group, byte) is correct as long as both operands use the same one.  The weight
// side picks the one that is cheapest to produce from the packed words, and the
// quantiser writes the workspace image of X^ to match:
//   a K step is 64 values; lane l = lr + 16 kg owns two chunks of 8 values,
//   chunk c at k = 64 s + 16 kg + 8 c (one 16x16x64 MFMA a step), or, when g %
//   64 == 32 (SPLIT), at k = 64 s + 32 c + 8 kg: then bytes 0..7 of all lanes are
//   the step's first 32 values and bytes 8..15 the second, and the step is two
//   16x16x32 MFMAs with a group boundary allowed between them;
//   inside a chunk byte p holds value klocal<B>(p):
//     4-bit: w & 0x0f0f0f0f and (w >> 4) & 0x0f0f0f0f, even nibbles then odd;
//     2-bit: four masks of the chunk's 16 bits; 8-bit: word ^ 0x80808080, in
//     order; 3-bit: eight shifts of the chunk's 24 bits, in order.
// The image: per (tile of 16 rows, step) 64 lanes x 16 bytes, so a wave loads an
// A operand as one contiguous KB; xsum as [tile][G][16 rows], a lane's four
// output rows being one 16-byte load.
//
// GEMM: one kernel for every T, the tiles of qmxact.hip: four waves own BM rows x
// 64 features, BM = 16 (T <= 32, waves side by side) or 64 (2 x 2 waves of 32 x
// 32).  Operands go from global memory straight into MFMA registers, no LDS:
// every wave reads different weight words (its own features), and the A tile is
// one coalesced KB per wave and step that two waves share through L2 / L1 -- an
// LDS stage would add a barrier per step to save that one re-read.  Four steps'
// operands are in flight ahead of the MFMAs.  K is split over blockIdx.z at
// multiples of a group (and of a step) while the tiles alone do not fill the
// device; the partial sums are added in ascending order by iact_reduce_kernel,
// which applies the row scale after the sum as the contract has it.
#include "../../include/truncgptq.h"
#include "common.h"
#include "qunpack.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int IA_TILE = 64;     // output features per workgroup
constexpr int IA_KS = 64;       // K step
constexpr int IA_TARGET_WGS = 512;
constexpr int IA_MIN_STEPS = 4;
constexpr int IA_SMALL_T = 32;  // rows up to which the 16-row tile is used
constexpr int IA_MAX_GROUPS = 8192;  // the quantiser keeps a row's group sums in LDS

// value index (0..7) inside a chunk that byte p of the chunk's operand holds
template <int B>
__host__ __device__ constexpr int klocal(int p) {
  if constexpr (B == 4) return 2 * (p & 3) + (p >> 2);
  else if constexpr (B == 2) return 2 * (p >> 2) + ((p >> 1) & 1) + 4 * (p & 1);
  else return p;
}

// offset inside a step of chunk c of lane group kg
__host__ __device__ inline int chunk_k(bool split, int kg, int c) {
  return split ? 32 * c + 8 * kg : 16 * kg + 8 * c;
}

// ---------------------------------------------------------------------------
// the quantiser: one workgroup per row, one thread per unit of 32 columns
// ---------------------------------------------------------------------------
template <int DT>
__device__ inline void load_unit(const uint16_t *__restrict__ src, int xvec, float (&x)[32]) {
  uint32_t h[16];
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
#pragma unroll
  for (int i = 0; i < 32; ++i) x[i] = from_bits<DT>(uint16_t(h[i >> 1] >> (16 * (i & 1))));
}

// B == 0: the ABI's image, xq T x n with row stride ldq, xs T, xsum T x G
// (nullable).  B in {2, 3, 4, 8}: the GEMM's workspace image described above.
template <int DT, int B>
__global__ __launch_bounds__(256) void quant_i8_kernel(const uint16_t *__restrict__ X, int64_t ldx,
                                                       int n, int g, int xvec, int split,
                                                       int8_t *__restrict__ xq, int64_t ldq,
                                                       int qvec, float *__restrict__ xs,
                                                       int32_t *__restrict__ xsum) {
  extern __shared__ int32_t gsum[];  // G group sums
  __shared__ float wmax[4];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int units = n / 32, G = n / g;
  const uint16_t *src = X + int64_t(row) * ldx;
  float x[32];
  float a = 0.f;
  for (int u = tid; u < units; u += 256) {
    load_unit<DT>(src + u * 32, xvec, x);
#pragma unroll
    for (int i = 0; i < 32; ++i) a = fmaxf(a, fabsf(x[i]));
  }
  for (int o = 32; o; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
  if ((tid & 63) == 0) wmax[tid >> 6] = a;
  for (int i = tid; i < G; i += 256) gsum[i] = 0;
  __syncthreads();
  a = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
  const float s = a / 127.f;
  const int steps = tg::cdiv(n, IA_KS);
  for (int u = tid; u < units; u += 256) {  // the second read of the row comes from cache
    load_unit<DT>(src + u * 32, xvec, x);
    int q[32], sum = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const float r = a > 0.f ? rintf(x[i] / s) : 0.f;
      q[i] = int(fminf(fmaxf(r, -127.f), 127.f));
      sum += q[i];
    }
    atomicAdd(&gsum[u * 32 / g], sum);  // integer, LDS: the order cannot change the result
    if constexpr (B == 0) {
      int8_t *dst = xq + int64_t(row) * ldq + u * 32;
      if (qvec) {
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          w[i] = uint32_t(q[4 * i] & 255) | (uint32_t(q[4 * i + 1] & 255) << 8) |
                 (uint32_t(q[4 * i + 2] & 255) << 16) | (uint32_t(q[4 * i + 3] & 255) << 24);
        reinterpret_cast<u32x4 *>(dst)[0] = u32x4{w[0], w[1], w[2], w[3]};
        reinterpret_cast<u32x4 *>(dst)[1] = u32x4{w[4], w[5], w[6], w[7]};
      } else {
#pragma unroll
        for (int i = 0; i < 32; ++i) dst[i] = int8_t(q[i]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {  // the unit's four chunks
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int p = 0; p < 8; ++p)
          w[p >> 2] |= uint32_t(q[8 * j + klocal<B>(p)] & 255) << (8 * (p & 3));
        const int k0 = u * 32 + j * 8, r = (k0 >> 3) & 7;
        const int kg = split ? r & 3 : r >> 1, c = split ? r >> 2 : r & 1;
        const int64_t ts = int64_t(row >> 4) * steps + (k0 >> 6);  // (tile, step)
        *reinterpret_cast<u32x2 *>(xq + ((ts * 64 + (row & 15) + 16 * kg) * 16 + 8 * c)) =
            u32x2{w[0], w[1]};
      }
    }
  }
  if (tid == 0) xs[row] = s;
  __syncthreads();
  if (!xsum) return;
  for (int i = tid; i < G; i += 256) {
    if constexpr (B == 0) xsum[int64_t(row) * G + i] = gsum[i];
    else xsum[(int64_t(row >> 4) * G + i) * 16 + (row & 15)] = gsum[i];
  }
}

template <int B>
void launch_quant(hipStream_t st, const void *X, int x_dtype, int T, int64_t ldx, int n, int g,
                  bool split, int8_t *xq, int64_t ldq, float *xs, int32_t *xsum) {
  const int xvec = (reinterpret_cast<uintptr_t>(X) % 16 == 0 && ldx % 8 == 0) ? 1 : 0;
  const int qvec = (reinterpret_cast<uintptr_t>(xq) % 16 == 0 && ldq % 16 == 0) ? 1 : 0;
  const size_t lds = size_t(n / g) * sizeof(int32_t);
  const uint16_t *Xp = static_cast<const uint16_t *>(X);
  if (x_dtype == TG_F16)
    hipLaunchKernelGGL((quant_i8_kernel<TG_F16, B>), dim3(T), dim3(256), lds, st, Xp, ldx, n, g,
                       xvec, int(split), xq, ldq, qvec, xs, xsum);
  else
    hipLaunchKernelGGL((quant_i8_kernel<TG_BF16, B>), dim3(T), dim3(256), lds, st, Xp, ldx, n, g,
                       xvec, int(split), xq, ldq, qvec, xs, xsum);
}

// ---------------------------------------------------------------------------
// the GEMM
// ---------------------------------------------------------------------------
// packed words that hold a chunk's 8 values
template <int B>
constexpr int chunk_words() { return (B == 3 || B == 8) ? 2 : 1; }

// a chunk's words -> its 8 operand bytes.  sh: 2-bit, the chunk's half of its
// word; 3-bit, where its 24 bits start in the word pair.
template <int B>
__device__ inline u32x2 expand(const uint32_t (&w)[chunk_words<B>()], int sh) {
  if constexpr (B == 4) {
    return u32x2{w[0] & 0x0f0f0f0fu, (w[0] >> 4) & 0x0f0f0f0fu};
  } else if constexpr (B == 8) {
    return u32x2{w[0] ^ 0x80808080u, w[1] ^ 0x80808080u};
  } else if constexpr (B == 2) {
    const uint32_t h = (w[0] >> sh) & 0xffffu;
    return u32x2{(h & 0x0303u) | (((h >> 2) & 0x0303u) << 16),
                 ((h >> 4) & 0x0303u) | (((h >> 6) & 0x0303u) << 16)};
  } else {
    const uint32_t v = uint32_t(((uint64_t(w[1]) << 32) | w[0]) >> sh);
    u32x2 r = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i >> 2] |= ((v >> (3 * i)) & 7u) << (8 * (i & 3));
    return r;
  }
}

// operands of one K step of a wave: MI row tiles of X^, NJ feature tiles of packed words
template <int B, int MI, int NJ>
struct IFrag {
  u32x4 a[MI];
  uint32_t b[NJ][2][chunk_words<B>()];
};

// what a fold needs of one group: z' and the scale of the lane's feature, xsum of its rows
template <int MI, int NJ>
struct GroupPar {
  int z[NJ];
  float s[NJ];
  i32x4 xsum[MI];
};

// Steps [blockIdx.z * sps, + sps) of the K range; sps covers whole groups.
// part == nullptr (one split): the row scale, the bias and the output rounding
// happen here; otherwise the f32 sums over the split's groups go to part[z][T][m].
template <int B, bool SPLIT, int MI, int NJ, int WR, int WC, int NS>
__global__ __launch_bounds__(256) void qiact_kernel(
    const int8_t *__restrict__ xq, const float *__restrict__ xs, const int32_t *__restrict__ xsum,
    int T, const uint32_t *__restrict__ qw, const uint32_t *__restrict__ qz,
    const void *__restrict__ sc, int sc_dt, int m, int n, int g, int sps, float *__restrict__ part,
    const void *__restrict__ bias, int bias_dt, void *__restrict__ Y, int y_dt, int64_t ldy) {
  static_assert(WR * WC == 4 && NJ * WC * 16 == IA_TILE && NS % 2 == 0);
  constexpr int BM = 16 * MI * WR;
  constexpr int NW = chunk_words<B>();
  constexpr int NA = MI * NJ == 1 ? 2 : 1;  // one tile a wave: two accumulators take turns
  constexpr int OFF = B == 8 ? 128 : 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave / WC, wc = wave % WC;
  const int lr = lane & 15, kg = lane >> 4;
  const int row0 = blockIdx.y * BM + wr * MI * 16, col0 = blockIdx.x * IA_TILE + wc * NJ * 16;
  const int steps = tg::cdiv(n, IA_KS), G = n / g, nzw = m * B / 32;
  const int s0 = blockIdx.z * sps, s1 = min(steps, s0 + sps);
  const int kend = min(n, s1 * IA_KS);  // a group boundary

  // the lane's two chunks: offset inside a step, word rows inside a step's 2 B rows
  int kc[2], wrow[2][NW], sh[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    kc[c] = chunk_k(SPLIT, kg, c);
    sh[c] = 0;
    if constexpr (B == 4) {
      wrow[c][0] = kc[c] >> 3;
    } else if constexpr (B == 8) {
      wrow[c][0] = kc[c] >> 2, wrow[c][1] = wrow[c][0] + 1;
    } else if constexpr (B == 2) {
      wrow[c][0] = kc[c] >> 4, sh[c] = 16 * ((kc[c] >> 3) & 1);
    } else {  // 24 j bits into the unit's three words
      const int j = (kc[c] >> 3) & 3, wi = (3 * j) >> 2;
      wrow[c][0] = 3 * (kc[c] >> 5) + wi, wrow[c][1] = 3 * (kc[c] >> 5) + min(wi + 1, 2);
      sh[c] = (24 * j) & 31;
    }
  }

  i32x4 acc[NA][MI][NJ];
  f32x4 accf[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      accf[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int p = 0; p < NA; ++p) acc[p][i][j] = i32x4{0, 0, 0, 0};
    }

  // Row tiles past T and features past m load nothing, and no chunk at or past
  // kend is read on either side.  Rows past T inside the last tile of 16 are
  // whatever the workspace held: they reach only output rows that are not stored.
  auto fetch = [&](int s, IFrag<B, MI, NJ> &f) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int tile = (row0 >> 4) + i;
      const u32x4 *src = reinterpret_cast<const u32x4 *>(xq) + (int64_t(tile) * steps + s) * 64 + lane;
      f.a[i] = (s < s1 && tile * 16 < T) ? *src : u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int o = col0 + j * 16 + lr;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const bool v = o < m && s * IA_KS + kc[c] < kend;
#pragma unroll
        for (int w = 0; w < NW; ++w)
          f.b[j][c][w] = v ? qw[(int64_t(s) * 2 * B + wrow[c][w]) * m + o] : 0u;
      }
    }
  };

  auto group_par = [&](int gi, GroupPar<MI, NJ> &p) {
    const bool gv = gi * g < kend;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int o = col0 + j * 16 + lr;
      const bool v = gv && o < m;
      p.z[j] = v ? zero_value(qz + int64_t(gi) * nzw, o, B) - OFF : 0;
      p.s[j] = v ? scale_value(sc, sc_dt, int64_t(gi) * m + o) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int tile = (row0 >> 4) + i;
      p.xsum[i] = (gv && tile * 16 < T)
                      ? reinterpret_cast<const i32x4 *>(xsum)[(int64_t(tile) * G + gi) * 4 + kg]
                      : i32x4{0, 0, 0, 0};
    }
  };

  // D = acc - z' xsum (|xsum| <= 127 * 65536 fits the 24-bit multiply), accf +=
  // float(D) * scale; C/D layout of the 16x16 MFMAs: col = lane & 15, row = 4 kg + reg
  auto fold = [&](const GroupPar<MI, NJ> &p) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          int d = acc[0][i][j][e];
          if constexpr (NA == 2) d += acc[1][i][j][e];
          d -= __mul24(p.z[j], p.xsum[i][e]);
          accf[i][j][e] += float(d) * p.s[j];
        }
#pragma unroll
        for (int q = 0; q < NA; ++q) acc[q][i][j] = i32x4{0, 0, 0, 0};
      }
  };

  int gi = int(int64_t(s0) * IA_KS / g), knext = (gi + 1) * g;  // the open group and its end
  GroupPar<MI, NJ> gp;
  group_par(gi, gp);
  auto close_group = [&](int kdone) {
    if (kdone != knext || kdone > kend) return;
    fold(gp);
    ++gi, knext += g;
    group_par(gi, gp);  // in flight until the next fold
  };

  auto mma = [&](int s, const IFrag<B, MI, NJ> &f, int par) {
    u32x2 bv[NJ][2];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int c = 0; c < 2; ++c) bv[j][c] = expand<B>(f.b[j][c], sh[c]);
    if constexpr (!SPLIT) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const i32x4 av = {int(f.a[i][0]), int(f.a[i][1]), int(f.a[i][2]), int(f.a[i][3])};
          const i32x4 bw = {int(bv[j][0][0]), int(bv[j][0][1]), int(bv[j][1][0]), int(bv[j][1][1])};
          i32x4 &c = acc[NA == 2 ? par : 0][i][j];
          c = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bw, c, 0, 0, 0);
        }
      close_group((s + 1) * IA_KS);
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int64_t av = int64_t((uint64_t(f.a[i][2 * h + 1]) << 32) | f.a[i][2 * h]);
            const int64_t bw = int64_t((uint64_t(bv[j][h][1]) << 32) | bv[j][h][0]);
            i32x4 &c = acc[NA == 2 ? h : 0][i][j];
            c = __builtin_amdgcn_mfma_i32_16x16x32_i8(av, bw, c, 0, 0, 0);
          }
        close_group(s * IA_KS + 32 * (h + 1));
      }
    }
  };

  // a ring of NS steps' operands in registers, indexed at compile time: the
  // loads of step s + NS - 1 are issued before the MFMAs of step s
  IFrag<B, MI, NJ> f[NS];
#pragma unroll
  for (int i = 0; i < NS - 1; ++i) fetch(s0 + i, f[i]);
  for (int s = s0; s < s1; s += NS) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      fetch(s + i + NS - 1, f[(i + NS - 1) % NS]);
      if (s + i < s1) mma(s + i, f[i], i & 1);
    }
  }

#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = col0 + j * 16 + lr;
      if (col >= m) continue;
      const float bv = (bias && !part) ? load_as_float(bias, bias_dt, col) : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = row0 + i * 16 + 4 * kg + e;
        if (row >= T) continue;
        if (part) {
          part[(int64_t(blockIdx.z) * T + row) * m + col] = accf[i][j][e];
        } else {
          const float v = __fmul_rn(accf[i][j][e], xs[row]);
          store_from_float(Y, y_dt, int64_t(row) * ldy + col, bias ? __fadd_rn(v, bv) : v);
        }
      }
    }
}

// Y[t, r] = round(xs[t] * sum_s part[s][t][r] (ascending s) + bias[r])
__global__ __launch_bounds__(256) void iact_reduce_kernel(const float *__restrict__ part, int S,
                                                          int T, int m,
                                                          const float *__restrict__ xs,
                                                          const void *__restrict__ bias,
                                                          int bias_dt, void *__restrict__ Y,
                                                          int y_dt, int64_t ldy) {
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= int64_t(T) * m) return;
  const int t = int(idx / m), r = int(idx - int64_t(t) * m);
  float v = part[idx];
  for (int s = 1; s < S; ++s) v += part[int64_t(s) * T * m + idx];
  v = __fmul_rn(v, xs[t]);
  if (bias) v = __fadd_rn(v, load_as_float(bias, bias_dt, r));
  store_from_float(Y, y_dt, int64_t(t) * ldy + r, v);
}

int act_rows(int T) { return T <= IA_SMALL_T ? 16 : 64; }

// g % 64 == 32: a group boundary falls inside a step
bool split_step(int g) { return g % IA_KS != 0; }

// K steps per workgroup: a multiple of the steps that end on a group boundary
// (g / 64, or g / 32 where two groups make a whole number of steps).  One split
// once the output tiles alone fill the device, otherwise enough for
// ~IA_TARGET_WGS workgroups of at least IA_MIN_STEPS steps.  Per-channel
// weights (g = n) are one group and never split.
int act_steps_per_split(int T, int m, int n, int g) {
  const int nstep = tg::cdiv(n, IA_KS);
  const int unit = split_step(g) ? g / 32 : g / IA_KS;
  const int64_t tiles = int64_t(tg::cdiv(m, IA_TILE)) * tg::cdiv(T, act_rows(T));
  int64_t S = (IA_TARGET_WGS + tiles - 1) / tiles;
  const int s_max = nstep / IA_MIN_STEPS > 1 ? nstep / IA_MIN_STEPS : 1;
  if (S > s_max) S = s_max;
  return tg::cdiv(tg::cdiv(nstep, S), unit) * unit;
}

struct ActLayout {
  int8_t *xq;
  float *xs, *part;
  int32_t *xsum;
  int sps, S;
};

template <class A>
ActLayout act_layout(A &a, int T, int m, int n, int g) {
  ActLayout l;
  const size_t tiles = size_t(tg::cdiv(T, 16)), nstep = size_t(tg::cdiv(n, IA_KS));
  l.sps = act_steps_per_split(T, m, n, g);
  l.S = tg::cdiv(nstep, l.sps);
  l.xq = a.template take_aligned<int8_t>(tiles * nstep * 1024, 256);
  l.xs = a.template take_aligned<float>(size_t(T), 256);
  l.xsum = a.template take_aligned<int32_t>(tiles * size_t(n / g) * 16, 256);
  l.part = l.S > 1 ? a.template take_aligned<float>(size_t(l.S) * T * m, 256) : nullptr;
  return l;
}

bool group_ok(int n, int g) {
  return g > 0 && g % 32 == 0 && n % g == 0 && g <= 65536 && n / g <= IA_MAX_GROUPS;
}
constexpr const char *GROUP_MSG =
    "group must be a multiple of 32 that divides n, at most 65536, with at most 8192 groups";

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" int tg_quant_act_i8(void *stream, const void *X, int x_dtype, int T, int64_t stride_x,
                               int n, int group, int8_t *xq, int64_t stride_q, float *xs,
                               int32_t *xsum) {
  TG_ARG(X, 2, "null X");
  TG_ARG(x_dtype == TG_F16 || x_dtype == TG_BF16, 3, "x_dtype must be TG_F16 or TG_BF16");
  TG_ARG(T > 0, 4, "T <= 0");
  TG_ARG(n > 0 && n % 32 == 0, 6, "n must be a positive multiple of 32");
  TG_ARG(stride_x >= n, 5, "stride_x < n");
  const int g = group > 0 ? group : n;
  TG_ARG(group_ok(n, g), 7, GROUP_MSG);
  TG_ARG(xq, 8, "null xq");
  TG_ARG(stride_q >= n, 9, "stride_q < n");
  TG_ARG(xs, 10, "null xs");
  launch_quant<0>((hipStream_t)stream, X, x_dtype, T, stride_x, n, g, false, xq, stride_q, xs, xsum);
  TG_LAUNCHED();
  return 0;
}

extern "C" size_t tg_qgemm_act_workspace_size(int T, int m, int n, int group) {
  const int g = group > 0 ? group : n;
  if (T <= 0 || m <= 0 || n < 32 || n % 32 || !group_ok(n, g)) return 0;
  tg::Sizer sz;
  act_layout(sz, T, m, n, g);
  return sz.off;
}

extern "C" int tg_qgemm_act(void *stream, const void *X, int x_dtype, int T, int64_t stride_x,
                            const int32_t *qweight, const int32_t *qzeros, const void *scales,
                            int scale_dtype, int m, int n, int group, int w_bits, int act_fmt,
                            const void *bias, int bias_dtype, void *Y, int y_dtype,
                            int64_t stride_y, void *ws, size_t ws_bytes) {
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
  TG_ARG(group_ok(n, g), 12, GROUP_MSG);
  TG_ARG(act_fmt == TG_ACT_INT8, 14, "act_fmt must be TG_ACT_INT8");
  TG_ARG(!bias || bias_dtype == TG_F16 || bias_dtype == TG_BF16 || bias_dtype == TG_F32, 16,
         "bias_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(Y, 17, "null Y");
  TG_ARG(y_dtype == TG_F16 || y_dtype == TG_BF16 || y_dtype == TG_F32, 18,
         "y_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(stride_y >= m, 19, "stride_y < m");
  const int BM = act_rows(T);
  TG_ARG(tg::cdiv(T, BM) <= 65535, 4, "T too large");
  TG_ARG(ws, 20, "null workspace");
  tg::Arena arena(ws, ws_bytes);
  const ActLayout l = act_layout(arena, T, m, n, g);
  TG_WS(arena);
  hipStream_t st = (hipStream_t)stream;
  const bool split = split_step(g);
  with_bits(w_bits, [&](auto b) {
    launch_quant<b.value>(st, X, x_dtype, T, stride_x, n, g, split, l.xq, n, l.xs, l.xsum);
  });
  TG_LAUNCHED();
  const dim3 grid(tg::cdiv(m, IA_TILE), tg::cdiv(T, BM), l.S);
  const uint32_t *qw = reinterpret_cast<const uint32_t *>(qweight);
  const uint32_t *qz = reinterpret_cast<const uint32_t *>(qzeros);
#define TG_IA(B_, SP_, MI_, NJ_, WR_, WC_)                                                        \
  hipLaunchKernelGGL((qiact_kernel<B_, SP_, MI_, NJ_, WR_, WC_, 4>), grid, dim3(256), 0, st, l.xq, \
                     l.xs, l.xsum, T, qw, qz, scales, scale_dtype, m, n, g, l.sps, l.part, bias,   \
                     bias_dtype, Y, y_dtype, stride_y)
#define TG_IA_TILE(B_, SP_)               \
  do {                                    \
    if (BM == 16) TG_IA(B_, SP_, 1, 1, 1, 4); \
    else TG_IA(B_, SP_, 2, 2, 2, 2);      \
  } while (0)
  with_bits(w_bits, [&](auto b) {
    if (split) TG_IA_TILE(b.value, true);
    else TG_IA_TILE(b.value, false);
  });
#undef TG_IA_TILE
#undef TG_IA
  TG_LAUNCHED();
  if (l.S > 1) {
    hipLaunchKernelGGL(iact_reduce_kernel, dim3(tg::cdiv(int64_t(T) * m, 256)), dim3(256), 0, st,
                       l.part, l.S, T, m, l.xs, bias, bias_dtype, Y, y_dtype, stride_y);
    TG_LAUNCHED();
  }
  return 0;
}
