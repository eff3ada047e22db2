// Shared by the grouped packed GEMMs (qgrouped.hip, qgroupedact.hip): how a
// workgroup finds its (expert, slot range) from the device-side offsets, the
// host's bound on the number of such tiles, and the split-K reduction that
// applies row_scale.
#pragma once
#include "../../include/truncgptq.h"
#include "common.h"
#include "qdtype.h"

namespace {

constexpr int GR_MAX_E = 256;      // one thread of the workgroup per expert in find_work

// ---------------------------------------------------------------------------
// Work tile `t` of the call, when every expert's slots are cut into runs of
// `run`: thread e counts expert e's runs, an inclusive scan over the workgroup
// (shuffles inside a wave, four wave totals through LDS) gives every expert's
// first tile, and the one expert whose range holds t publishes (e, first slot,
// end slot).  e = -1: the call has fewer than t + 1 tiles.  Counts and slot
// ranges are clamped to [0, R], so a malformed offsets array cannot carry an
// index out of the buffers.  All 256 threads call it.
// ---------------------------------------------------------------------------
struct Work { int e, s0, s1; };

__device__ inline Work find_work(const int32_t *__restrict__ offsets, int E, int R, int run,
                                 int t) {
  __shared__ int wsum[4];
  __shared__ int found[3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int o = 0, c = 0;
  if (tid < E) {
    o = min(max(offsets[tid], 0), R);
    c = min(max(offsets[tid + 1], 0), R) - o;
    if (c < 0) c = 0;
  }
  const int nt = (c + run - 1) / run;
  int incl = nt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(incl, d, 64);
    if (lane >= d) incl += v;
  }
  if (lane == 63) wsum[wave] = incl;
  if (tid == 0) found[0] = -1;
  __syncthreads();
  int excl = incl - nt;
  for (int w = 0; w < wave; ++w) excl += wsum[w];
  if (t >= excl && t < excl + nt) {  // nt > 0 here: at most one thread
    found[0] = tid;
    found[1] = o + (t - excl) * run;
    found[2] = min(o + c, o + (t - excl + 1) * run);
  }
  __syncthreads();
  return Work{found[0], found[1], found[2]};
}

// upper bound on the number of tiles: sum_e ceil(c_e / run) <= (R + E (run - 1)) / run,
// and no more than R (a tile holds at least one slot)
int64_t tile_bound(int R, int E, int run) {
  const int64_t b = (int64_t(R) + int64_t(E) * (run - 1)) / run;
  return b < R ? b : R;
}

// Y[i, r] = round(row_scale[i] * sum_s part[s][i][r]), s ascending
__global__ __launch_bounds__(256) void qgrouped_reduce_kernel(const float *__restrict__ part, int S,
                                                              int R, int m,
                                                              const float *__restrict__ row_scale,
                                                              void *__restrict__ Y, int y_dt,
                                                              int64_t ldy) {
  const int64_t idx = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= int64_t(R) * m) return;
  const int i = int(idx / m), r = int(idx - int64_t(i) * m);
  float v = part[idx];
  for (int s = 1; s < S; ++s) v += part[int64_t(s) * R * m + idx];
  if (row_scale) v *= row_scale[i];
  store_from_float(Y, y_dt, int64_t(i) * ldy + r, v);
}

}  // namespace
