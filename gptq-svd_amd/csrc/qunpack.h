// Shared by the packed GEMMs that unpack weights themselves (qlinear.hip,
// qgrouped.hip): the AutoGPTQ bit stream and the MXFP4 pair decoded one unit of
// 32 values at a time, and the 16x16x32 MFMA on raw 16-bit operands.  The
// layouts are described at the top of qlinear.hip.  qiact.hip takes the bit
// stream and the host's choice of code width from here too.
#pragma once
#include <type_traits>

#include "qdtype.h"

namespace {

// ---- the code widths (host) ---------------------------------------------------
inline bool bits_ok(int b) { return b == 2 || b == 3 || b == 4 || b == 8; }

// f(std::integral_constant<int, B>{}) for the run-time w_bits, so that B can
// pick a template instance.  Callers have checked bits_ok; any other width
// runs as 8.
template <class F>
inline void with_bits(int w_bits, F &&f) {
  switch (w_bits) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

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
// The kernels take a format parameter: FMT_INT decodes (code - zero) *
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

// ---- the MFMA tile geometry both tile kernels use -----------------------------
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

}  // namespace
