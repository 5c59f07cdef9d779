// The "S16" pre-split activation format (include/accflow_hip.h): hi = fp16(x 2^ASHIFT), lo = fp16(x 2^ASHIFT - hi), two
// channels per 32-bit word; |x 2^ASHIFT| >= 65520 (what fp16 rounds to infinity) or NaN belongs in
// accflow_conv_desc.guard.  The ONLY place that knows the arithmetic: every producer and consumer calls these.  What
// stays at a site: masking of absent channels, store addressing and the atomicOr on the guard.
#pragma once
#include "accflow_hip.h"

typedef unsigned mu32x4 __attribute__((ext_vector_type(4)));

constexpr float S16_SCALE = (float)(1 << ACCFLOW_F16_ASHIFT);
constexpr float S16_LIMIT = 65520.0f;
constexpr unsigned S16_LIMIT_BITS = 0x477FF000u;   // S16_LIMIT as an integer: |x| compares as its bit pattern does
static_assert(__builtin_bit_cast(unsigned, S16_LIMIT) == S16_LIMIT_BITS, "S16_LIMIT_BITS");

// range check of SCALED values: true beyond fp16's range and for NaN
__device__ __forceinline__ bool s16_bad(float a) { return !(fabsf(a) < S16_LIMIT); }
__device__ __forceinline__ bool s16_bad2(float a, float b) { return !(fabsf(a) < S16_LIMIT) | !(fabsf(b) < S16_LIMIT); }

// two SCALED values -> one word of the hi plane, one of the lo plane (packed converts, round to nearest each)
__device__ __forceinline__ void s16_split2(float a, float b, unsigned& hi, unsigned& lo) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const f2 v = {a, b};
  const h2 hq = __builtin_convertvector(v, h2);
  const f2 back = __builtin_convertvector(hq, f2);
  const f2 r = {a - back[0], b - back[1]};
  const h2 lq = __builtin_convertvector(r, h2);
  hi = __builtin_bit_cast(unsigned, hq);
  lo = __builtin_bit_cast(unsigned, lq);
}

// one SCALED value -> its hi (low 16 bits) and lo (high 16 bits) halves (scalar converts: conv_stem.hip)
__device__ __forceinline__ unsigned s16_split1(float a) {
  const _Float16 hq = (_Float16)a;
  const _Float16 lq = (_Float16)(a - (float)hq);
  return (unsigned)__builtin_bit_cast(unsigned short, hq) | ((unsigned)__builtin_bit_cast(unsigned short, lq) << 16);
}

// One 16-byte chunk pair: the 8 channel values x[OFF .. OFF + 7] of one pixel times the power of two `s`; `bad` collects
// the range check.
template <int OFF = 0, int N>
__device__ __forceinline__ void s16_split8(const float (&x)[N], mu32x4& hi, mu32x4& lo, bool& bad, float s = S16_SCALE) {
  unsigned h[4], l[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = x[OFF + 2 * j] * s, b = x[OFF + 2 * j + 1] * s;
    bad |= s16_bad2(a, b);
    s16_split2(a, b, h[j], l[j]);
  }
  hi = mu32x4{h[0], h[1], h[2], h[3]};
  lo = mu32x4{l[0], l[1], l[2], l[3]};
}

// the value of half q (0: low, 1: high 16 bits) of a hi / lo word pair
__device__ __forceinline__ float s16_join(unsigned hi, unsigned lo, int q) {
  const _Float16 h = __builtin_bit_cast(_Float16, (unsigned short)(hi >> (16 * q)));
  const _Float16 l = __builtin_bit_cast(_Float16, (unsigned short)(lo >> (16 * q)));
  return ((float)h + (float)l) * (1.0f / S16_SCALE);
}
