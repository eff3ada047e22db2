// Sketch mode: Y += Omega X with a Gaussian Omega that is never stored
// (the reference's Sketcher.hook_fn, gptq_utils.py:184-202: a torch.randn of
// rank x tokens followed by an fp32 addmm_).
//
// omega(seed, r, g) -- r the sketch row, g the global token index -- is a pure
// function (contract in include/truncgptq.h):
//   Philox4x32-10, key = (seed lo, seed hi),
//   counter = (g lo, g hi, (r >> 7) * 32 + (r & 31), 0);
//   its four outputs x0..x3 belong to the rows that differ from r only in
//   j = (r >> 5) & 3:  (x0, x1) -> j = 0 (cos), 1 (sin); (x2, x3) -> j = 2, 3;
//   Box-Muller: u1 = ((xa >> 8) + 1) 2^-24 in (0, 1], u2 = (xb >> 8) 2^-24 in
//   [0, 1) (both exact in fp32), rad = sqrtf(-2 logf(u1)),
//   omega = rad * cospif(2 u2) | rad * sinpif(2 u2).
// One lane of the fused kernel owns sketch rows R0 + i + 32 j (R0 a multiple of
// 128, i = lane & 31), i.e. exactly the four rows of one Philox call, so a
// call feeds the A operand of four 32 x 32 x 2 MFMAs per column block.
//
// Fused kernel: workgroup tile 512 sketch rows x 128 columns, four waves of
// 128 x 128 (4 x 4 blocks of 32 x 32, 256 accumulator registers loaded from
// Y), K tile of 32 tokens of X staged through LDS as fp32 (exact conversion).
// Per two tokens a lane generates its four omegas once and issues 16 MFMAs.
// v_mfma_f32_32x32x2_f32 with the accumulator as C is bit for bit the fmaf
// chain acc = fmaf(omega, x, acc) in ascending token order, so there is no
// token split, no atomics and no workspace, and the result does not depend on
// how the tokens are divided into calls.
#pragma clang fp contract(off)
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "../../include/truncgptq.h"
#include "common.h"

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

struct Omega4 {
  float v[4];
};

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = uint64_t(0xD2511F53u) * c[0];
  const uint64_t p1 = uint64_t(0xCD9E8D57u) * c[2];
  const uint32_t n0 = uint32_t(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n2 = uint32_t(p0 >> 32) ^ c[3] ^ k1;
  c[0] = n0;
  c[1] = uint32_t(p1);
  c[2] = n2;
  c[3] = uint32_t(p0);
}

// The four omegas of token g and row group rg (rows (rg >> 5) * 128 + (rg & 31) + 32 j).
__device__ __forceinline__ Omega4 omega4(uint32_t k0, uint32_t k1, uint64_t g, uint32_t rg) {
  uint32_t c[4] = {uint32_t(g), uint32_t(g >> 32), rg, 0u};
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Omega4 o;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = float((c[2 * p] >> 8) + 1u) * 0x1p-24f;
    const float u2 = float(c[2 * p + 1] >> 8) * 0x1p-23f;  // 2 u2: the angle in half turns
    const float rad = sqrtf(-2.0f * logf(u1));
    float s, co;
    sincospif(u2, &s, &co);
    o.v[2 * p] = rad * co;
    o.v[2 * p + 1] = rad * s;
  }
  return o;
}

__device__ __forceinline__ uint32_t row_group(int r) {
  return (uint32_t(r) >> 7) * 32u + (uint32_t(r) & 31u);
}

__global__ __launch_bounds__(256) void sketch_omega_kernel(uint32_t k0, uint32_t k1, int64_t t0,
                                                           int rank, int64_t T,
                                                           float *__restrict__ Om, int64_t ldo) {
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int r = blockIdx.y;
  if (t >= T || r >= rank) return;
  const Omega4 o = omega4(k0, k1, uint64_t(t0 + t), row_group(r));
  const int j = (r >> 5) & 3;
  Om[int64_t(r) * ldo + t] = j == 0 ? o.v[0] : j == 1 ? o.v[1] : j == 2 ? o.v[2] : o.v[3];
}

constexpr int TM = 512, TN = 128, TK = 32, LDX = TN + 32;  // LDX: rows k, k + 1 on disjoint banks

template <class XT>
__device__ __forceinline__ float to_f32(XT v);
template <>
__device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <>
__device__ __forceinline__ float to_f32<__half>(__half v) { return __half2float(v); }
template <>
__device__ __forceinline__ float to_f32<__hip_bfloat16>(__hip_bfloat16 v) {
  return __bfloat162float(v);
}

template <class XT>
__global__ __launch_bounds__(256) void sketch_accum_kernel(const XT *__restrict__ X, int64_t T,
                                                           int n, int64_t ldx, uint32_t k0,
                                                           uint32_t k1, int64_t t0,
                                                           float *__restrict__ Y, int rank,
                                                           int64_t ldy) {
  __shared__ float Xs[TK][LDX];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l32 = lane & 31, h = lane >> 5;
  const int tn = blockIdx.x * TN;
  const int R0 = blockIdx.y * TM + wave * 128;
  const uint32_t rg = row_group(R0 + l32);
  const bool idle = R0 >= rank;  // wave-uniform: no row of this wave's tile exists

  // Y addressing: the workgroup tile's base plus a 32-bit lane offset (the host
  // checks 512 * ldy * 4 < 2^32).  Lanes past an edge read a clamped, valid
  // address; they are never stored.
  float *const Yt = Y + int64_t(blockIdx.y) * TM * ldy + tn;
  const int rows_here = rank - blockIdx.y * TM;  // >= 1
  const int lr0 = wave * 128 + 4 * h;            // tile-local row of (i = 0, r = 0)
  const uint32_t ld32 = uint32_t(ldy);
  uint32_t coff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) coff[j] = uint32_t(min(tn + j * 32 + l32, n - 1) - tn);

  floatx16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int lr = lr0 + i * 32 + (r & 3) + 8 * (r >> 2);
      const uint32_t ro = __umul24(uint32_t(min(lr, rows_here - 1)), ld32);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j][r] = Yt[ro + coff[j]];
      // a finished row block goes to the accumulator registers at once (left to
      // itself the allocator keeps all 256 values in VGPRs here and spills)
      if (r == 15) {
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "+a"(acc[i][j]));
      }
    }

  // staging: thread -> column tid & 127, tokens (tid >> 7) + 2 u
  const int sc = tid & (TN - 1);
  const int sr = __builtin_amdgcn_readfirstlane(tid >> 7);
  const bool col_ok = tn + sc < n;
  const uint32_t xoff = uint32_t(min(tn + sc, n - 1));
  XT stage[TK / 2];
  auto fetch = [&](int64_t kb) {
#pragma unroll
    for (int u = 0; u < TK / 2; ++u) {
      const int64_t t = kb + sr + 2 * u;  // wave-uniform
      const XT v = (X + min(t, T - 1) * ldx)[xoff];
      stage[u] = (col_ok && t < T) ? v : XT(0.0f);
    }
  };
  // omega of token t for this lane's four rows; K padding multiplies 0 by 0
  auto gen = [&](int64_t t) {
    Omega4 o = omega4(k0, k1, uint64_t(t0 + t), rg);
    if (t >= T) o.v[0] = o.v[1] = o.v[2] = o.v[3] = 0.0f;
    return o;
  };
  fetch(0);
  // Software pipeline: the omegas of step s + 1 are generated (VALU) between
  // the 16 MFMAs of step s; the sched_group_barrier sequence spells out the
  // interleave, which the scheduler does not find by itself.
  Omega4 o = gen(h);
  for (int64_t kb = 0; kb < T; kb += TK) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TK / 2; ++u) Xs[sr + 2 * u][sc] = to_f32<XT>(stage[u]);
    __syncthreads();
    if (kb + TK < T) fetch(kb + TK);
    if (idle) continue;
    const int steps = int(min(int64_t(TK), T - kb) + 1) >> 1;  // whole steps only
    for (int ks = 0; ks < steps; ++ks) {
      const int kk = 2 * ks;
      float b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Xs[kk + h][j * 32 + l32];
      const Omega4 on = gen(kb + kk + 2 + h);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.v[i], b[j], acc[i][j], 0, 0, 0);
      o = on;
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);  // the LDS reads of b
      __builtin_amdgcn_sched_group_barrier(0x002, 16, 0);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 13, 0);  // 13 VALU
      }
    }
  }

  if (idle) return;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (r == 0) {  // row blocks leave the accumulator registers one at a time
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "+a"(acc[i][j]));
      }
      const int lr = lr0 + i * 32 + (r & 3) + 8 * (r >> 2);
      const uint32_t ro = __umul24(uint32_t(lr), ld32);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (lr < rows_here && tn + j * 32 + l32 < n) Yt[ro + coff[j]] = acc[i][j][r];
    }
}

}  // namespace

extern "C" int tg_sketch_omega(void *stream, uint64_t seed, int64_t t0, int rank, int64_t T,
                               float *Omega, int64_t ldo) {
  TG_ARG(t0 >= 0, 3, "t0 < 0");
  TG_ARG(rank > 0, 4, "rank <= 0");
  TG_ARG(T >= 0 && T <= INT64_MAX - t0, 5, "T < 0 or t0 + T overflows");
  if (T == 0) return 0;
  TG_ARG(Omega, 6, "null Omega");
  TG_ARG(ldo >= T, 7, "ldo < T");
  TG_ARG(rank <= 65535 && (T + 255) / 256 <= INT32_MAX, 4, "rank > 65535 (tests / tools only)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned((T + 255) / 256), unsigned(rank));
  sketch_omega_kernel<<<grid, 256, 0, st>>>(uint32_t(seed), uint32_t(seed >> 32), t0, rank, T,
                                            Omega, ldo);
  TG_LAUNCHED();
  return 0;
}

extern "C" int tg_sketch_accum(void *stream, const void *X, int x_dtype, int64_t T, int n,
                               int64_t ldx, uint64_t seed, int64_t t0, float *Y, int rank,
                               int64_t ldy) {
  TG_ARG(x_dtype == TG_F16 || x_dtype == TG_BF16 || x_dtype == TG_F32, 3,
         "x_dtype must be TG_F16, TG_BF16 or TG_F32");
  TG_ARG(n > 0, 5, "n <= 0");
  TG_ARG(t0 >= 0, 8, "t0 < 0");
  TG_ARG(T >= 0 && T <= INT64_MAX - t0, 4, "T < 0 or t0 + T overflows");
  TG_ARG(ldx >= n, 6, "ldx < n");
  TG_ARG(rank > 0, 10, "rank <= 0");
  TG_ARG(ldy >= n, 11, "ldy < n");
  TG_ARG(ldy < (int64_t(1) << 21), 11, "ldy >= 2^21");
  TG_ARG(Y, 9, "null Y");
  if (T == 0) return 0;
  TG_ARG(X, 2, "null X");
  TG_ARG(tg::cdiv(rank, TM) <= 65535, 10, "rank > 65535 * 512");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(unsigned(tg::cdiv(n, TN)), unsigned(tg::cdiv(rank, TM)));
  const uint32_t k0 = uint32_t(seed), k1 = uint32_t(seed >> 32);
  if (x_dtype == TG_F16)
    sketch_accum_kernel<__half><<<grid, 256, 0, st>>>(static_cast<const __half *>(X), T, n, ldx,
                                                      k0, k1, t0, Y, rank, ldy);
  else if (x_dtype == TG_BF16)
    sketch_accum_kernel<__hip_bfloat16><<<grid, 256, 0, st>>>(
        static_cast<const __hip_bfloat16 *>(X), T, n, ldx, k0, k1, t0, Y, rank, ldy);
  else
    sketch_accum_kernel<float><<<grid, 256, 0, st>>>(static_cast<const float *>(X), T, n, ldx, k0,
                                                     k1, t0, Y, rank, ldy);
  TG_LAUNCHED();
  return 0;
}
