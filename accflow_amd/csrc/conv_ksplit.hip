// The split-K reduction of the direct convolution kernel: conv2d_direct.hip launches Z partial sums into d.kws, these add them.
// out = epilogue(act(sum_z part[z] + bias)): the K-parts are added in the fixed order z = 0, 1, ... (deterministic).  The
// three kernels differ in their thread shape and in how they store the S16 copy; the value and the epilogue are one body each.
#include "conv_common.h"

namespace {

// the activated value of (b, ch, px) from `sum`, the sum of its K-parts: row scale and bias, the GRU epilogues' context addend
__device__ __forceinline__ float ksplit_value(const accflow_conv_desc& d, float sum, int b, int ch, int px, int OHW) {
  float v = fmaf(sum, d.wscale16 ? d.wscale16[(d.wsplit_bs ? (long long)b * d.CoutPad : 0) + ch] : 1.0f, d.bias ? d.bias[ch] : 0.0f);
  if (d.pre && (d.epi == ACCFLOW_EPI_GRU_ZR || d.epi == ACCFLOW_EPI_GRU_Q)) v += d.pre[b * d.pre_bs + (long long)ch * OHW + px];
  return apply_act(v, d.act);
}

// the epilogue's result for the value v of (b, ch, px), written to the fp32 destination where there is one
__device__ __forceinline__ float ksplit_epilogue(const accflow_conv_desc& d, float v, int b, int ch, int px, int OHW) {
  if (d.cb) {  // channel-block scatter (STORE / ACCUM): see accflow_conv_desc.cb
    const int blk = ch / d.cb;
    const long long oc = (long long)(ch - blk * d.cb) * OHW + px;
    const float r = d.epi == ACCFLOW_EPI_ACCUM ? d.e0[b * d.e0_bs + blk * d.e0_cbs + oc] + v : v;
    if (d.out) d.out[b * d.out_bs + blk * d.out_cbs + oc] = r;
    return r;
  }
  const long long o = (long long)ch * OHW + px;
  const int half = d.Cout >> 1;
  const bool rrow = d.epi == ACCFLOW_EPI_GRU_ZR && ch >= half;   // r gate rows: r * h into out2
  float r = v;
  switch (d.epi) {
    case ACCFLOW_EPI_RES_RELU: r = fmaxf(d.e0[b * d.e0_bs + o] + v, 0.0f); break;
    case ACCFLOW_EPI_GRU_ZR:
      if (rrow) r = v * d.e0[b * d.e0_bs + o - (long long)half * OHW];
      break;
    case ACCFLOW_EPI_GRU_Q: {
      const float z = d.e1[b * d.e1_bs + o], h = d.e0[b * d.e0_bs + o];
      r = gru_blend(z, h, v);
    } break;
    case ACCFLOW_EPI_ACCUM: r = d.e0[b * d.e0_bs + o] + v; break;
    default: break;
  }
  if (rrow) {
    if (d.out2) d.out2[b * d.out2_bs + o - (long long)half * OHW] = r;
  } else if (d.out) {
    d.out[b * d.out_bs + o] = r;
  }
  return r;
}

// one thread per output element (the form used when no S16 copy is requested: measured 9.6 vs 13.3 us per launch for
// the octet-per-thread form below on the batch-1 fusion chain)
__global__ __launch_bounds__(256) void conv_ksplit_reduce_kernel(const accflow_conv_desc d, int Z) {
  const int OHW = d.OH * d.OW;
  const long long n = (long long)d.B * d.Cout * OHW;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int px = (int)(i % OHW);
  const int ch = (int)((i / OHW) % d.Cout);
  const int b = (int)(i / ((long long)OHW * d.Cout));
  float v = d.kws[i];
  for (int z = 1; z < Z; ++z) v += d.kws[(long long)z * n + i];
  ksplit_epilogue(d, ksplit_value(d, v, b, ch, px, OHW), b, ch, px, OHW);
}

// Thread = (batch item, octet of 8 output channels, pixel): the fp32 stores of the 8 channels are 8 coalesced stores
// along the pixels, and the 8 results are exactly one chunk of the S16 copy (accflow_conv_desc.out16) when requested.
__global__ __launch_bounds__(256) void conv_ksplit_reduce_s16_kernel(const accflow_conv_desc d, int Z) {
  const int OHW = d.OH * d.OW;
  const int O = (d.Cout + 7) >> 3;
  const long long n = (long long)d.B * d.Cout * OHW;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)d.B * O * OHW) return;
  const int px = (int)(i % OHW);
  const int oct = (int)((i / OHW) % O);
  const int b = (int)(i / ((long long)OHW * O));
  const int half = d.Cout >> 1;
  const bool zr = d.epi == ACCFLOW_EPI_GRU_ZR;
  float res[8];   // what the S16 copy holds: 0 for an absent channel and for the z rows of GRU_ZR
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int ch = oct * 8 + j;
    res[j] = 0.0f;
    if (ch >= d.Cout) continue;
    const long long e = ((long long)b * d.Cout + ch) * OHW + px;
    float v = d.kws[e];
    for (int z = 1; z < Z; ++z) v += d.kws[(long long)z * n + e];
    const float r = ksplit_epilogue(d, ksplit_value(d, v, b, ch, px, OHW), b, ch, px, OHW);
    if (d.cb || !zr || ch >= half) res[j] = r;
  }
  if (!d.out16) return;
  // S16 copy: GRU_ZR -> the r*h channels (octets counted from Cout/2, which is a multiple of 8), else all channels
  const int c16 = oct * 8 - (zr ? half : 0);
  if (c16 < 0) return;
  const int n16 = zr ? half : d.Cout;
  const int nvalid = min(8, ((n16 + 1) & ~1) - c16);   // whole channel pairs only (accflow_conv_desc.out16)
  mu32x4 hi, lo;
  bool bad = false;
  s16_split8(res, hi, lo, bad);
  unsigned* base = reinterpret_cast<unsigned*>(d.out16) + b * d.out16_bs;
  int o16 = c16 >> 3;
  if (d.cb) {
    base += (long long)(c16 / d.cb) * d.out16_cbs;
    o16 = (c16 % d.cb) >> 3;
  }
  unsigned* ph = base + (((long long)(o16 * 2 + 0)) * OHW + px) * 4;
  unsigned* pl = base + (((long long)(o16 * 2 + 1)) * OHW + px) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (2 * k < nvalid) { ph[k] = hi[k]; pl[k] = lo[k]; }
  if (bad && d.guard) atomicOr(d.guard, 1);
}

// The same for the common case of the batch-1 fusion chain on pre-split tensors (and the GMA aggregation: per-item row scales,
// channel-block scatter) - every octet complete, not the GRU_ZR form - with a thread per (batch item, 4-channel group, pixel): half the serial loads per thread and
// twice the threads of the octet form above (480 workgroups for 128 channels x 7 680 pixels left most CUs idle: 15 us per
// launch, 0.9 ms per sequence for the chain's 60 reduces, profiles/r04_kernel_stats_bench_1stream.txt).  A lane writes its 4
// channels' 8 bytes into each term's chunk, the conv epilogue's store pattern.  (cb % 32 == 0: the 4 channels share a block.)
__global__ __launch_bounds__(256) void conv_ksplit_reduce_s16q_kernel(const accflow_conv_desc d, int Z) {
  const int OHW = d.OH * d.OW;
  const int Q = d.Cout >> 2;
  const long long n = (long long)d.B * d.Cout * OHW;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)d.B * Q * OHW) return;
  const int px = (int)(i % OHW);
  const int q = (int)((i / OHW) % Q);
  const int b = (int)(i / ((long long)OHW * Q));
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = d.kws[((long long)b * d.Cout + q * 4 + j) * OHW + px];
  for (int z = 1; z < Z; ++z)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] += d.kws[(long long)z * n + ((long long)b * d.Cout + q * 4 + j) * OHW + px];
  float res[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) res[j] = ksplit_epilogue(d, ksplit_value(d, v[j], b, q * 4 + j, px, OHW), b, q * 4 + j, px, OHW);
  unsigned hi[2], lo[2];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float a = res[2 * k] * S16_SCALE, c = res[2 * k + 1] * S16_SCALE;
    bad |= s16_bad2(a, c);
    s16_split2(a, c, hi[k], lo[k]);
  }
  unsigned* base = reinterpret_cast<unsigned*>(d.out16) + b * d.out16_bs;
  int oct = q >> 1;
  const int w0 = (q & 1) * 2;
  if (d.cb) {
    base += (long long)((q * 4) / d.cb) * d.out16_cbs;
    oct = ((q * 4) % d.cb) >> 3;
  }
  unsigned* ph = base + (((long long)(oct * 2 + 0)) * OHW + px) * 4 + w0;
  unsigned* pl = base + (((long long)(oct * 2 + 1)) * OHW + px) * 4 + w0;
  typedef unsigned u2_ __attribute__((ext_vector_type(2)));
  *reinterpret_cast<u2_*>(ph) = u2_{hi[0], hi[1]};
  *reinterpret_cast<u2_*>(pl) = u2_{lo[0], lo[1]};
  if (bad && d.guard) atomicOr(d.guard, 1);
}

}  // namespace

int conv_ksplit_reduce_launch(const accflow_conv_desc& d, int Z, hipStream_t st) {
  if (d.out16 && !(d.Cout & 7) && !(d.cb & 7) && d.epi != ACCFLOW_EPI_GRU_ZR) {
    const long long nthr = (long long)d.B * (d.Cout / 4) * d.OH * d.OW;
    hipLaunchKernelGGL(conv_ksplit_reduce_s16q_kernel, dim3(cdiv(nthr, 256)), dim3(256), 0, st, d, Z);
  } else if (d.out16) {
    const long long nthr = (long long)d.B * ((d.Cout + 7) / 8) * d.OH * d.OW;
    hipLaunchKernelGGL(conv_ksplit_reduce_s16_kernel, dim3(cdiv(nthr, 256)), dim3(256), 0, st, d, Z);
  } else {
    const long long nout = (long long)d.B * d.Cout * d.OH * d.OW;
    hipLaunchKernelGGL(conv_ksplit_reduce_kernel, dim3(cdiv(nout, 256)), dim3(256), 0, st, d, Z);
  }
  ACCFLOW_RETURN_LAUNCH_STATUS();
}
