// The numeric rules of the weight / operand packs, each written ONCE (device only; conv_pack.hip, conv2d_s16m.hip and
// gma_alt.hip pack with them, so their packs agree bit for bit by construction):
//   the fp16 row scale   wscale16 = 2^-(k + ACCFLOW_F16_ASHIFT), k such that the row maximum * 2^k lies in [2^10, 2^11);
//   the term splits      three bf16 terms; fp16 hi + lo with a zero third slot; 8 values -> one 16-byte hi and lo chunk;
//   the k-table entry    {channel inside its source, ky, kx, source}, padding entries never in range.
// (s16_split8 of s16_format.h / split8_bf16 of conv_common.h are the K-loop kernels' splits of ACTIVATIONS: vector converts, a range check.)
#pragma once
#include <hip/hip_runtime.h>
#include "accflow_hip.h"

typedef unsigned pack_u32x4 __attribute__((ext_vector_type(4)));

// maximum of m over the 256 threads of a workgroup, delivered to all of them (every thread of the workgroup calls it)
__device__ __forceinline__ float pack_block_max256(float m) {
  __shared__ float red[256];
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  return red[0];
}

// row maximum m -> wscale16 (k = 0 for an all-zero / non-finite row)
__device__ __forceinline__ float pack_row_scale16(float m) {
  int k = 0;
  if (m > 0.0f && m < 3.0e38f) {
    int e;
    frexpf(m, &e);  // m = f * 2^e, f in [0.5, 1)  ->  m * 2^(11 - e) in [2^10, 2^11)
    k = 11 - e;
    if (k > 100) k = 100;
    if (k < -100) k = -100;
  }
  return ldexpf(1.0f, -(k + ACCFLOW_F16_ASHIFT));
}
// the factor 2^k that takes a weight of the row to its packed value: exact power-of-two scaling, |w * 2^k| < 2^11
__device__ __forceinline__ float pack_row_mul16(float wscale16) { return ldexpf(1.0f, -ACCFLOW_F16_ASHIFT) / wscale16; }

// r -> three bf16 terms at dst[0], dst[per_term], dst[2 per_term]
__device__ __forceinline__ void pack_store_bf16x3(unsigned short* __restrict__ dst, long long per_term, float r) {
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const __bf16 b = (__bf16)r;
    dst[t * per_term] = __builtin_bit_cast(unsigned short, b);
    r -= (float)b;
  }
}

// r (row-scaled) -> fp16 hi, lo and a zero third slot
__device__ __forceinline__ void pack_store_f16x2z(unsigned short* __restrict__ dst, long long per_term, float r) {
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const _Float16 hq = t < 2 ? (_Float16)r : (_Float16)0.0f;
    dst[t * per_term] = __builtin_bit_cast(unsigned short, hq);
    r -= (float)hq;
  }
}

// 8 values x[q] * gmul * mul -> fp16 hi / lo, one 16-byte chunk each
__device__ __forceinline__ void pack_hilo8(const float (&x)[8], float gmul, float mul, pack_u32x4& hv, pack_u32x4& lv) {
  unsigned short hi[8], lo[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    float rr = x[q] * gmul * mul;
    const _Float16 h = (_Float16)rr;
    rr -= (float)h;
    const _Float16 l = (_Float16)rr;
    hi[q] = __builtin_bit_cast(unsigned short, h);
    lo[q] = __builtin_bit_cast(unsigned short, l);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    hv[q] = (unsigned)hi[2 * q] | ((unsigned)hi[2 * q + 1] << 16);
    lv[q] = (unsigned)lo[2 * q] | ((unsigned)lo[2 * q + 1] << 16);
  }
}

// k-table entry of reduction index k = (channel c of the concatenated sources, ky, kx); !live: a padding entry
__device__ __forceinline__ int4 pack_ktab_entry(bool live, int c, int ky, int kx, int C0) {
  int4 e;
  if (live) { e.x = c < C0 ? c : c - C0; e.y = ky; e.z = kx; e.w = c < C0 ? 0 : 1; }
  else { e.x = 0; e.y = 1 << 20; e.z = 1 << 20; e.w = 0; }
  return e;
}
