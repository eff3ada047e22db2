// The gemv regime of tg_qgemm, shared by qlinear.hip (X staged in column order)
// and qgidx.hip (X staged through col_perm): the geometry, the regime switch,
// and everything a workgroup does once its K chunk of X lies in LDS as fp32.
// Both kernels run this one body, so their results agree bit for bit whenever
// the staged values do.
#pragma once
#include <cstdlib>
#include <cstring>

#include "qunpack.h"

namespace {

constexpr int GV_FEAT = 64;          // output features per workgroup (one per lane)
constexpr int GV_WAVES = 4;          // K sub-slices of a workgroup
constexpr int GV_MAX_UNITS = 16;     // K chunk of a workgroup <= 512 values (X in LDS as fp32)
constexpr int GV_MAX_T = 16;         // rows the gemv regime takes
constexpr int GV_AUTO_T = 4;         // rows up to which TG_QGEMM=auto picks it (measured)
constexpr int GV_TARGET_WGS = 1024;  // ~4 workgroups per CU of a 256-CU device

// units of 32 values per workgroup along K; the number of K splits follows
inline int gemv_units_per_wg(int m, int n) {
  const int units = n / 32, tiles = tg::cdiv(m, GV_FEAT);
  int S = tg::cdiv(GV_TARGET_WGS, tiles);
  const int s_max = tg::cdiv(units, GV_WAVES), s_min = tg::cdiv(units, GV_MAX_UNITS);
  if (S > s_max) S = s_max;
  if (S < s_min) S = s_min;
  if (S < 1) S = 1;
  return tg::cdiv(units, S);
}

// TG_QGEMM (read per call): 0 auto (gemv up to T = 4, mfma above), 1 gemv (T <= 16), 2 mfma
inline int qgemm_mode() {
  const char *e = getenv("TG_QGEMM");
  if (e && strcmp(e, "gemv") == 0) return 1;
  if (e && strcmp(e, "mfma") == 0) return 2;
  return 0;
}

// After the barrier that follows the staging of xs[t][k] = x[t, column of
// stream position u0 * 32 + k] (rows t >= T zero): the wave's units against xs,
// the waves' sums added in wave order through LDS, part[blockIdx.y][t][r] written.
template <int B, int DT, int TT, int FMT>
__device__ __forceinline__ void gemv_accumulate(
    const float (&xs)[TT][GV_MAX_UNITS * 32], float (&red)[GV_WAVES][TT][GV_FEAT], int T,
    const uint32_t *__restrict__ qw, const uint32_t *__restrict__ qz, const void *__restrict__ sc,
    int sc_dt, int m, int g, int u0, int u1, float *__restrict__ part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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

}  // namespace
