// Shared by the packed-inference files (qlinear.hip, qmxact.hip): the 16-bit
// operand / output types as raw bits, and the split-K reduction that finishes
// both files' partial sums.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "../../include/truncgptq.h"
#include "common.h"

namespace {

// ---- 16-bit operand types as raw bits --------------------------------------
template <int DT>
__device__ inline uint16_t to_bits(float v) {
  if constexpr (DT == TG_F16) {
    return __half_as_ushort(__float2half_rn(v));
  } else {
    return __builtin_bit_cast(uint16_t, static_cast<__bf16>(v));  // RNE (v_cvt_pk_bf16_f32)
  }
}

template <int DT>
__device__ inline float from_bits(uint16_t h) {
  if constexpr (DT == TG_F16) return __half2float(__ushort_as_half(h));
  else return __uint_as_float(uint32_t(h) << 16);
}

__device__ inline float load_as_float(const void *p, int dt, int64_t i) {
  if (dt == TG_F16) return from_bits<TG_F16>(static_cast<const uint16_t *>(p)[i]);
  if (dt == TG_BF16) return from_bits<TG_BF16>(static_cast<const uint16_t *>(p)[i]);
  return static_cast<const float *>(p)[i];
}

__device__ inline void store_from_float(void *p, int dt, int64_t i, float v) {
  if (dt == TG_F16) static_cast<uint16_t *>(p)[i] = to_bits<TG_F16>(v);
  else if (dt == TG_BF16) static_cast<uint16_t *>(p)[i] = to_bits<TG_BF16>(v);
  else static_cast<float *>(p)[i] = v;
}

// Y[t, r] = round(sum_s part[s][t][r] (ascending s) + bias[r])
__global__ __launch_bounds__(256) void qgemv_reduce_kernel(const float *__restrict__ part, int S,
                                                           int T, int m,
                                                           const void *__restrict__ bias,
                                                           int bias_dt, void *__restrict__ Y,
                                                           int y_dt, int64_t ldy) {
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= int64_t(T) * m) return;
  const int t = int(idx / m), r = int(idx - int64_t(t) * m);
  float v = part[idx];
  for (int s = 1; s < S; ++s) v += part[int64_t(s) * T * m + idx];
  if (bias) v += load_as_float(bias, bias_dt, r);
  store_from_float(Y, y_dt, int64_t(t) * ldy + r, v);
}

}  // namespace
