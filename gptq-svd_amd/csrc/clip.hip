// A7c: Hessian-weighted clip search for the static-group scale / zero
// (tg_group_params_clip; no counterpart in the reference, whose
// Quantizer.find_params, gptq_utils.py:249-266, is candidate 0 of the search).
//
// Contract (include/truncgptq.h restates it for callers).  W is m x n f32,
// groups are g consecutive original columns, h = col_weight (n f32 >= 0, null
// = all ones).  Candidates i = 0 .. steps shrink the group's range by
//   p = 1.0f - float(i) / float(grid)                       (two f32 ops)
// asym, mn / mx the group's min / max:
//   lo = mn < 0 ? p * mn : mn      hi = mx > 0 ? p * mx : mx
//   d  = max(hi - lo, 1e-5f)       s  = d / maxq
//   z  = clamp(rintf(-lo / s), 0, maxq)
// sym, a the group's max |w|:
//   s  = max(p * a, 1e-5f) / maxq  z  = 0
// objective over the group's elements c (the tail / RTN rounding rule,
// gptq_utils.py:552-553):
//   q = clamp(rintf(w_c / s + z), minq, maxq)   dq = (q - z) * s   e = w_c - dq
//   J_i = sum_c double(h_c) * (double(e) * double(e))       (fp64)
// Every f32 operation above is one correctly rounded IEEE operation in the
// order written (no contraction; true division).  The chosen candidate is the
// smallest i with minimal J_i: only a strictly smaller J replaces the best so
// far, so steps = 0 is tg_group_params bit for bit and J_chosen <= J_0.
//
// Summation order of J: a group is shared by L lanes (L a power of two <= 64
// chosen from g alone); lane `sub` adds its elements sub, sub + L, ... in
// ascending order, then the L partial sums are combined by an xor butterfly
// (offsets L/2 .. 1).  The order is the same for every candidate and every
// call; there are no atomics.
//
// Shape of the kernel.  Pass 1 reduces mn / mx (or absmax) over the group.
// Candidates are then evaluated in register-blocked chunks of NB (16, 4, 1):
// the NB (s, z) pairs and NB fp64 partial sums live in registers, and each
// element of the lane is used NB times with the candidate loop innermost.
// Groups of up to 16 * 64 columns keep the lane's <= 16 elements (and their
// weights, widened once) in registers, so W is read once; wider groups (the
// per-row g = n case) stream the lane's elements from cache once per chunk.
// Groups narrower than 16 * 64 share a wave: g <= 16 is one lane per group,
// g = 128 eight lanes per group.
#pragma clang fp contract(off)

#include <climits>

#include "../../include/truncgptq.h"
#include "common.h"

namespace {

constexpr int EPL = 16;  // elements a lane holds on the register path

struct Cand {
  float s, z;
};

__device__ __forceinline__ Cand candidate(int i, int grid, bool sym, float mn, float mx,
                                          float maxq) {
  const float p = 1.0f - float(i) / float(grid);
  Cand c;
  if (sym) {
    float a = p * mx;
    a = a < 1e-5f ? 1e-5f : a;
    c.s = a / maxq;
    c.z = 0.0f;
  } else {
    const float lo = mn < 0.0f ? p * mn : mn;
    const float hi = mx > 0.0f ? p * mx : mx;
    float d = hi - lo;
    d = d < 1e-5f ? 1e-5f : d;
    c.s = d / maxq;
    float z = rintf(-lo / c.s);
    c.z = z < 0.0f ? 0.0f : (z > maxq ? maxq : z);
  }
  return c;
}

__device__ __forceinline__ double sq_err(float w, float s, float z, float minq, float maxq) {
  float q = rintf(w / s + z);
  q = fminf(fmaxf(q, minq), maxq);
  const float dq = (q - z) * s;
  const float e = w - dq;
  const double ed = double(e);
  return ed * ed;
}

template <bool REG>
__global__ __launch_bounds__(256) void clip_kernel(
    const float *__restrict__ W, int64_t stride_w, const float *__restrict__ h, int64_t units,
    int g, int G, int L, int sym, float maxq, float minq, int grid, int steps,
    float *__restrict__ scale, float *__restrict__ zero, int32_t *__restrict__ choice,
    double *__restrict__ objective) {
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  const int64_t unit = t / L;
  const int sub = int(t & (L - 1));
  // L divides 64, so a group's lanes sit in one wave and leave together
  if (unit >= units) return;
  const int64_t r = unit / G, gi = unit % G;
  const float *pw = W + r * stride_w + gi * g;
  const float *ph = h ? h + gi * g : nullptr;

  float w[EPL];
  double hd[EPL];
  int cnt = 0;
  float mn = INFINITY, mx = -INFINITY;
  if (REG) {
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const int c = sub + k * L;
      w[k] = 0.0f;
      hd[k] = 0.0;
      if (c < g) {
        w[k] = pw[c];
        hd[k] = ph ? double(ph[c]) : 1.0;
        cnt = k + 1;
      }
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      if (k < cnt) {
        if (sym) {
          mx = fmaxf(mx, fabsf(w[k]));
        } else {
          mn = fminf(mn, w[k]);
          mx = fmaxf(mx, w[k]);
        }
      }
    }
  } else {
    for (int c = sub; c < g; c += L) {
      const float v = pw[c];
      if (sym) {
        mx = fmaxf(mx, fabsf(v));
      } else {
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
      }
    }
  }
  for (int off = L >> 1; off > 0; off >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, off));
    mx = fmaxf(mx, __shfl_xor(mx, off));
  }

  int best = 0;
  double best_j = 0.0, j0 = 0.0;

  auto run = [&]<int NB>(int i0) {
    float s[NB], z[NB];
    double acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const Cand c = candidate(i0 + j, grid, sym != 0, mn, mx, maxq);
      s[j] = c.s;
      z[j] = c.z;
      acc[j] = 0.0;
    }
    if (REG) {
#pragma unroll
      for (int k = 0; k < EPL; ++k) {
        if (k < cnt) {
#pragma unroll
          for (int j = 0; j < NB; ++j)
            acc[j] = __builtin_fma(hd[k], sq_err(w[k], s[j], z[j], minq, maxq), acc[j]);
        }
      }
    } else {
      for (int c = sub; c < g; c += L) {
        const float v = pw[c];
        const double hv = ph ? double(ph[c]) : 1.0;
#pragma unroll
        for (int j = 0; j < NB; ++j)
          acc[j] = __builtin_fma(hv, sq_err(v, s[j], z[j], minq, maxq), acc[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      double a = acc[j];
      for (int off = L >> 1; off > 0; off >>= 1) a += __shfl_xor(a, off);
      if (i0 + j == 0) {
        j0 = a;
        best_j = a;
      } else if (a < best_j) {
        best_j = a;
        best = i0 + j;
      }
    }
  };

  int i0 = 0, rem = steps + 1;
  for (; rem >= 16; rem -= 16, i0 += 16) run.template operator()<16>(i0);
  for (; rem >= 4; rem -= 4, i0 += 4) run.template operator()<4>(i0);
  for (; rem >= 1; rem -= 1, i0 += 1) run.template operator()<1>(i0);

  if (sub == 0) {
    const Cand c = candidate(best, grid, sym != 0, mn, mx, maxq);
    scale[unit] = c.s;
    zero[unit] = c.z;
    if (choice) choice[unit] = best;
    if (objective) {
      objective[2 * unit] = j0;
      objective[2 * unit + 1] = best_j;
    }
  }
}

}  // namespace

extern "C" int tg_group_params_clip(void *stream, const float *W, int m, int n, int64_t stride_w,
                                    const float *col_weight, int group, int w_bits, int sym,
                                    int grid, int steps, float *scale, float *zero,
                                    int32_t *choice, double *objective) {
  TG_ARG(W, 2, "null W");
  TG_ARG(m > 0, 3, "m <= 0");
  TG_ARG(n > 0, 4, "n <= 0");
  TG_ARG(stride_w >= n, 5, "stride_w < n");
  const int g = group > 0 ? group : n;
  TG_ARG(n % g == 0, 7, "n % group_size != 0 (gptq_utils.py:253)");
  TG_ARG(w_bits >= 2 && w_bits <= 8, 8, "w_bits must be in [2, 8]");
  TG_ARG(grid >= 1, 10, "grid < 1");
  TG_ARG(steps >= 0 && steps < grid, 11, "steps must be in [0, grid)");
  TG_ARG(scale, 12, "null scale");
  TG_ARG(zero, 13, "null zero");
  const int G = n / g;
  const float maxq = sym ? float((1 << (w_bits - 1)) - 1) : float((1 << w_bits) - 1);
  const float minq = sym ? -maxq : 0.0f;
  int L = 1;
  while (L < 64 && tg::cdiv(g, L) > EPL) L <<= 1;
  const bool reg = tg::cdiv(g, L) <= EPL;
  const int64_t units = int64_t(m) * G;
  const int64_t blocks = (units * L + 255) / 256;
  TG_ARG(blocks <= INT_MAX, 3, "m * n / group is too large for one launch");
  hipLaunchKernelGGL(reg ? clip_kernel<true> : clip_kernel<false>, dim3((unsigned)blocks),
                     dim3(256), 0, (hipStream_t)stream, W, stride_w, col_weight, units, g, G, L,
                     sym, maxq, minq, grid, steps, scale, zero, choice, objective);
  TG_LAUNCHED();
  return 0;
}
